#!/usr/bin/env python
"""Launcher for subpopr's summariseClusteringResultsForAll (src/subpopr/R/summariseClusteringResults.R); the work is metasnv_amd/subpopr.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from metasnv_amd.subpopr import summarise_clustering_main as main

if __name__ == "__main__":
    main()
