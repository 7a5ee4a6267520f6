#!/usr/bin/env python3
"""VALU issue slots of a line range of a gfx950 assembly listing: every v_* instruction counts once, the half-rate ones of
profiles/r01_valu_issue_rates.txt twice.  Usage: isa_valu_slots.py FILE.s FIRST LAST [FIRST LAST ...] (1-based, inclusive).
Prints, per range, the instructions, the half-rate ones among them and the slots, then the commonest mnemonics."""
import collections
import re
import sys

HALF = re.compile(r"^v_(alignbit|alignbyte|perm_b32|lshlrev_b32|lshl_or|lshl_add|and_or|or3|add3|mad_u32_u24|mad_i32_i24|mul_u32_u24|"
                  r"mul_i32_i24|mul_lo|mul_hi|bfe|bfi|min3|max3|med3|min_i32|max_i32|min_u32|max_u32|cndmask|mbcnt|pk_|cvt_|sad_|"
                  r"dot|lshlrev_b64|lshrrev_b64|ashrrev_i64|mad_u64|readlane|readfirstlane|writelane)|_sdwa|_dpp")


def count(lines):
    n = half = 0
    names = collections.Counter()
    for ln in lines:
        t = ln.strip().split()
        if not t or not t[0].startswith("v_"):
            continue
        n += 1
        names[t[0]] += 1
        if HALF.search(t[0]):
            half += 1
    return n, half, names


def main():
    text = open(sys.argv[1]).read().split("\n")
    for a, b in zip(sys.argv[2::2], sys.argv[3::2]):
        n, half, names = count(text[int(a) - 1:int(b)])
        print("lines %s-%s: %d VALU, %d of them half rate, %d slots" % (a, b, n, half, n + half))
        print("   " + ", ".join("%s %d" % kv for kv in names.most_common(10)))


if __name__ == "__main__":
    main()
