#!/usr/bin/env python
"""Launcher for subpopr's useGenotypesToProfileSubpops (src/subpopr/R/profileSubpops.R) on one species' genotyping SNV frequencies in every sample; the work is metasnv_amd/subpopr.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from metasnv_amd.subpopr import profile_subpops_main as main

if __name__ == "__main__":
    main()
