#!/usr/bin/env python3
"""filter-abund.py on the MI355X path: see khmer_amd/scripts.py (filter_abund)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from khmer_amd.scripts import filter_abund, run  # noqa: E402

if __name__ == "__main__":
    run(filter_abund)
