#!/usr/bin/env python3
"""normalize-by-median.py on the MI355X path: see khmer_amd/scripts.py (normalize_by_median)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from khmer_amd.scripts import normalize_by_median, run  # noqa: E402

if __name__ == "__main__":
    run(normalize_by_median)
