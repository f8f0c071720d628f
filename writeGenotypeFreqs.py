#!/usr/bin/env python
"""Launcher for subpopr's writeGenotypeFreqs (src/subpopr/R/writeGenotypeFreqs.R) on one species' clustering and SNV frequency table; the work is metasnv_amd/subpopr.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from metasnv_amd.subpopr import write_genotype_freqs_main as main

if __name__ == "__main__":
    main()
