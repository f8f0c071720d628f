#!/usr/bin/env python
"""Launcher with the reference function's name and argument order (src/subpopr/R/correlateSubpopProfileWithGeneProfiles.R); the work is metasnv_amd/subpopr.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from metasnv_amd.subpopr import correlate_gene_profiles_main as main

if __name__ == "__main__":
    main()
