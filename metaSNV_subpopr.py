#!/usr/bin/env python
"""Launcher with the reference's name and options (metaSNV_subpopr.R); the work is metasnv_amd/subpopr_run.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from metasnv_amd.subpopr_run import main

if __name__ == "__main__":
    main()
