"""Diagnostics: what the compiler made of the publication of the exchange records (mgx_sweep.h, end of a segment of a resident
launch) in ONE sweep-kernel instantiation, from its listing.
usage: python tools/publication_listing.py [--flavor 1|2] [--kset 0|1|2] [-K 16] [--features 0|2|3] [--listing FILE.s] [extra hipcc flags ...]
Compiles magics_amd/csrc/mgx_sweep_inst.hip for that instantiation (or reads a listing made the same way) and finds the LOCAL
publication: the first run of agent-scope 16-byte buffer stores (`buffer_store_dwordx4 ... offen ... sc1`, not `sc0 sc1`) behind a
`; wave barrier`.  Its span runs from that barrier to the last of those stores — to the end of the innermost loop around them
where they sit in one.  Prints, for the span: whether it has a back edge (a store inside a loop deeper than the segment loop),
LDS reads, `s_waitcnt` that wait on lgkmcnt, v_mul_lo_u32, v_mul_hi_u32, v_cndmask_b32, s_and_saveexec_b64 and all instructions;
for the sharded flavour the same for the REMOTE publication (the system-scope stores, `sc0 sc1`); and for the whole listing the
lgkmcnt waits, v_mul_lo_u32, s_and_saveexec_b64, code length, scratch and spills.
Exit status 1 if the local publication of a constant-K instantiation has a back edge or more than two lgkmcnt waits."""
import argparse
import re
import sys

from gather_listing import blocks_of, listing

SPAN_OPS = ("ds_read", "lgkmcnt wait", "v_mul_lo_u32", "v_mul_hi_u32", "v_cndmask_b32", "s_and_saveexec_b64", "instructions")


def op_of(line):
    t = line.split(";")[0].split()
    return t[0] if t and not t[0].endswith(":") and not t[0].startswith(".") else ""


def count(lines, lo, hi):
    c = {k: 0 for k in SPAN_OPS}
    for l in lines[lo:hi]:
        op = op_of(l)
        if not op:
            continue
        c["instructions"] += 1
        if op.startswith("s_waitcnt"):
            c["lgkmcnt wait"] += "lgkmcnt" in l
        for k in ("ds_read", "v_mul_lo_u32", "v_mul_hi_u32", "v_cndmask_b32", "s_and_saveexec_b64"):
            c[k] += op.startswith(k)
    return c


def depth_of(lines, bl, i):
    """loop depth of the block that holds line i (1: the segment loop)"""
    b = next(b for b in bl if b["lo"] <= i < b["hi"])
    head = [lines[b["lo"]]]  # the label's line and the comment lines behind it ("Parent Loop ... Depth=1", "=> This Inner Loop Header: Depth=2")
    for l in lines[b["lo"] + 1:b["hi"]]:
        if not l.strip().startswith(";"):
            break
        head.append(l)
    own = [int(d) for l in head for d in re.findall(r"(?:Header=\S+|Loop Header:) Depth=(\d+)", l)]
    return max(own) if own else 0


def span_of(lines, bl, stores, barrier):
    """(first line, last line + 1, has a back edge) of a run of stores"""
    deep = max(depth_of(lines, bl, i) for i in stores)
    hi = stores[-1] + 1
    if deep >= 2:  # in a loop inside the segment loop: to the end of that loop's last block
        at = next(n for n, b in enumerate(bl) if b["lo"] <= stores[-1] < b["hi"])
        while at + 1 < len(bl) and depth_of(lines, bl, bl[at + 1]["lo"]) >= deep:
            at += 1
        hi = bl[at]["hi"]
    return barrier, hi, deep


def runs(lines, pred):
    """runs of lines that satisfy pred, a run ending where the next such line is more than 200 lines away"""
    idx = [i for i, l in enumerate(lines) if pred(l)]
    out = []
    for i in idx:
        if out and i - out[-1][-1] <= 200:
            out[-1].append(i)
        else:
            out.append([i])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flavor", type=int, default=1)
    ap.add_argument("--kset", type=int, default=1)
    ap.add_argument("-K", type=int, default=16)
    ap.add_argument("--features", type=int, default=3, choices=(0, 2, 3), help="the form: 0 lean, 2 with prior updates, 3 full")
    ap.add_argument("--listing")
    args, extra = ap.parse_known_args()
    path = args.listing or listing(args.flavor, args.kset, args.K, extra, args.features)
    lines = open(path).read().splitlines()
    bl = blocks_of(lines)
    barriers = [i for i, l in enumerate(lines) if l.strip() == "; wave barrier"]
    is_store = lambda l: op_of(l) == "buffer_store_dwordx4" and " offen" in l
    local = lambda l: is_store(l) and l.rstrip().endswith(" sc1") and " sc0 " not in l
    remote = lambda l: is_store(l) and l.rstrip().endswith("sc0 sc1")
    print(path)
    print(f"{'':20s} " + " ".join(f"{k:>19s}" for k in ("loop depth",) + SPAN_OPS))
    bad = False
    for name, pred in (("local publication", local), ("remote publication", remote)):
        rr = [r for r in runs(lines, pred) if any(b < r[0] for b in barriers)]
        if not rr:
            continue
        r = rr[0]
        barrier = max(b for b in barriers if b < r[0]) if name.startswith("local") else bl[next(n for n, b in enumerate(bl) if b["lo"] <= r[0] < b["hi"])]["lo"]
        lo, hi, deep = span_of(lines, bl, r, barrier)
        c = count(lines, lo, hi)
        print(f"{name:20s} {deep:19d} " + " ".join(f"{c[k]:19d}" for k in SPAN_OPS) + f"   (lines {lo + 1} - {hi}, {len(r)} stores)")
        if name.startswith("local") and args.K > 0 and (deep >= 2 or c["lgkmcnt wait"] > 2):
            bad = True
    whole = "\n".join(lines)
    c = count(lines, 0, len(lines))
    for k in ("lgkmcnt wait", "v_mul_lo_u32", "s_and_saveexec_b64"):
        print(f"{k:28s} {c[k]}")
    for key in ("codeLenInByte", ".private_segment_fixed_size", ".sgpr_spill_count", ".vgpr_spill_count"):
        m = re.search(re.escape(key) + r"\D+(\d+)", whole)
        print(f"{key.lstrip('.'):28s} {m.group(1) if m else '?'}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
