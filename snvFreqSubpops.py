#!/usr/bin/env python
"""Launcher for the numbers behind subpopr's SNV-frequency plots (src/subpopr/R/snvFreqPlot.R) on one species' filtered frequency table; the work is metasnv_amd/subpopr.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from metasnv_amd.subpopr import snv_freq_subpops_main as main

if __name__ == "__main__":
    main()
