#!/usr/bin/env python
"""Launcher for subpopr's computePCoA (src/subpopr/R/clustering.R) on one species' distance matrix; the work is metasnv_amd/subpopr.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from metasnv_amd.subpopr import pcoa_subpops_main as main

if __name__ == "__main__":
    main()
