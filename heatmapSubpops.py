#!/usr/bin/env python
"""Launcher for the row order of subpopr's report heatmaps (src/subpopr/inst/rmd/detailedSpeciesReport.rmd) on one species' distance matrix; the work is metasnv_amd/subpopr.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from metasnv_amd.subpopr import heatmap_subpops_main as main

if __name__ == "__main__":
    main()
