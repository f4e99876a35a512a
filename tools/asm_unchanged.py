#!/usr/bin/env python3
"""Build-machine guard of a change that must leave every kernel alone (no GPU needed): compares the gfx950 assembly kept by
two builds (knode-cosserat_amd/lib/asm/*.s).

    python tools/asm_unchanged.py <asm dir of the parent commit> <asm dir of this tree>

Part 1 of tools/tab_asm_compare.py on its own, with one rule more: every kernel of the parent build must be in this build
under the same name with the same resources, per-loop instruction census and instruction text, and this build must hold
no kernel the parent does not have.

Exit status 1 if a kernel is missing, new or different."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tab_asm_compare as tac  # noqa: E402

if __name__ == "__main__":
    sys.exit(1 if tac.part1(sys.argv, new_ok=False)[0] else 0)
