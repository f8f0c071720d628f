#!/usr/bin/env python
"""Launcher for subpopr's writeSubpopAbundSpeciesAbund (src/subpopr/R/writeSubpopAbund.R) on one species' subspecies frequencies and a species abundance table; the work is metasnv_amd/subpopr.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from metasnv_amd.subpopr import write_subpop_abund_main as main

if __name__ == "__main__":
    main()
