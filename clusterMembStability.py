#!/usr/bin/env python
"""Launcher for subpopr's getClusMembStability (src/subpopr/R/clusteringStability.R) on one species' clustering; the work is metasnv_amd/subpopr.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from metasnv_amd.subpopr import cluster_memb_stability_main as main

if __name__ == "__main__":
    main()
