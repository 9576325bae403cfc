#!/usr/bin/env python3
"""Compare two device assemblies of rssync_kernels.hip function by function: which kernels did a change of the device code
touch, and what did it cost them?

    cd rs-sync_amd/csrc && hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S rssync_kernels.hip -o new.s    (and old.s
    from the parent commit's tree); then: python tools/isa_compare.py old.s new.s [--json out.json]

Text against text: comments are dropped and the function numbers in local labels (.LBB230_15 -> .LBB_15) are masked, since
they shift with every function added before; nothing else is interpreted.  Prints the symbols only one side has, then one
line per function whose instructions differ: lines, VGPRs, SGPRs, LDS and private segment bytes, spill counts, old -> new.
Exit status 1 if the symbol sets differ, else 0."""
import argparse
import json
import re
import sys

START = re.compile(r"^([A-Za-z_$][\w$.]*):")
LABEL = re.compile(r"\.L([A-Za-z_]+)\d+(_\d+)?")
FIELDS = {"vgpr": ".amdhsa_next_free_vgpr", "sgpr": ".amdhsa_next_free_sgpr", "lds": ".amdhsa_group_segment_fixed_size",
          "private": ".amdhsa_private_segment_fixed_size"}


def functions(path):
    """-> {symbol: {"text": [instructions and labels], "vgpr": .., "sgpr": .., "lds": .., "private": .., spill counts}}"""
    out, name = {}, None
    meta = None
    for raw in open(path):
        line = raw.split(";")[0].strip()
        if meta is not None:                        # the metadata at the file's end: spill counts per kernel
            key, _, val = line.partition(":")
            if raw.startswith("    .name:"):        # a kernel's own (an argument's name is indented further)
                meta = out.get(val.strip(), {})
            elif key in (".sgpr_spill_count", ".vgpr_spill_count"):
                meta[key[1:]] = int(val)
            continue
        if line == ".amdgpu_metadata":
            meta = {}
        elif START.match(line):                     # (local labels start with a dot and do not match)
            name = START.match(line).group(1)
            if name.startswith("__hip_cuid_"):      # the compilation's id: a hash of the source text
                name = None
            else:
                out[name] = {"text": []}
        elif name is None:
            pass
        elif line.startswith(".Lfunc_end"):
            name = None
        elif line.startswith(".amdhsa_"):
            for key, word in FIELDS.items():
                if line.startswith(word + " "):
                    out[name][key] = int(line.split()[1])
        elif line and not line.startswith((".section", ".p2align", ".end_amdhsa_kernel")):
            out[name]["text"].append(LABEL.sub(lambda m: ".L%s%s" % (m.group(1), m.group(2) or ""), line))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--json", help="write the differing functions here as well")
    a = ap.parse_args()
    old, new = functions(a.old), functions(a.new)
    for side, names in (("old", sorted(set(old) - set(new))), ("new", sorted(set(new) - set(old)))):
        for n in names:
            print("only in %s: %s" % (side, n))
    rows = []
    for n in sorted(set(old) & set(new)):
        if old[n]["text"] != new[n]["text"]:
            row = {"name": n, "lines": [len(old[n]["text"]), len(new[n]["text"])]}
            for key in list(FIELDS) + ["sgpr_spill_count", "vgpr_spill_count"]:
                row[key] = [old[n].get(key), new[n].get(key)]
            rows.append(row)
            print("%s\n    " % n + "  ".join("%s %s -> %s" % (k, v[0], v[1]) for k, v in row.items() if k != "name"))
    print("%d functions old, %d new, %d in both differ" % (len(old), len(new), len(rows)))
    if a.json:
        json.dump(rows, open(a.json, "w"), indent=1)
    return 1 if set(old) != set(new) else 0


if __name__ == "__main__":
    sys.exit(main())
