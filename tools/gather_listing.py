"""Diagnostics: what the compiler made of gather_records (mgx_sweep.h) in ONE sweep-kernel instantiation, from its listing.
usage: python tools/gather_listing.py [--flavor 1|2] [--kset 0|1|2] [-K 16] [--features 0|2|3] [--listing FILE.s] [extra hipcc flags ...]
Compiles magics_amd/csrc/mgx_sweep_inst.hip for that instantiation (or reads a listing made the same way), finds the gather's
spin loop (the innermost loop around its `s_sleep 32`) and prints, per part of the gather, the instructions that are bookkeeping:
  front       the six blocks in front of the loop (addresses, first requests)
  look        the loop from its header to the pause
  re-request  the rest of the loop
  exit        the block behind it
and, for the whole listing, v_max_f64, the 64-bit address arithmetic, code length, scratch and spills.

It also CHECKS the in-place loads (ld16_into): between a load written in the source as an instruction and the wait behind it
(ld16_landed), no other instruction may name a register the load was aimed at — the compiler does not know the load is in
flight.  The check follows the listing's text, block by block, as the loop is laid out; exit status 1 if it finds one."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTED = ("v_mov_b64", "v_mov_b32", "v_add_u32", "v_cmp_ne_u32", "buffer_load_dwordx4", "s_waitcnt")


def listing(flavor, kset, k, extra, features=3):
    out = os.path.join(tempfile.mkdtemp(prefix="mgx_listing_"), f"sweep_f{flavor}_k{k}_feat{features}.s")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", f"-DMGX_FLAVOR={flavor}", f"-DMGX_KSET={kset}", f"-DMGX_FEAT={features}",
                    f"-DMGX_ONLY_K={k}", "-S", "--cuda-device-only", *extra, os.path.join(ROOT, "magics_amd", "csrc", "mgx_sweep_inst.hip"), "-o", out],
                   check=True, stderr=subprocess.DEVNULL)
    return out


def blocks_of(lines):
    """[(label, first line, last line + 1, loop header named in the label's comment or None)] of the kernel's basic blocks"""
    starts = [(i, m) for i, l in enumerate(lines) for m in [re.match(r"(\.LBB\d+_\d+):(.*)|; %bb\.(\d+):(.*)", l)] if m]
    out = []
    for n, (i, m) in enumerate(starts):
        end = starts[n + 1][0] if n + 1 < len(starts) else len(lines)
        label = m.group(1) or "%bb." + m.group(3)
        rest = "\n".join(lines[i:i + 4])
        h = re.search(r"Header=(BB\d+_\d+) Depth=(\d+)", rest)
        own = re.search(r"This Inner Loop Header: Depth=(\d+)", rest)
        out.append(dict(label=label, lo=i, hi=end, header=h.group(1) if h else None, is_header=bool(own)))
    return out


def regs(text):
    """VGPR numbers an instruction's text names"""
    found = set()
    for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", text):
        found.update(range(int(a), int(b) + 1))
    found.update(int(a) for a in re.findall(r"\bv(\d+)\b", text))
    return found


def count(lines, lo, hi):
    c = {k: 0 for k in COUNTED}
    for l in lines[lo:hi]:
        op = l.split()[0] if l.split() else ""
        for k in COUNTED:
            if op.startswith(k):
                c[k] += 1
    return c


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
    sleep = next((i for i, l in enumerate(lines) if re.match(r"\s+s_sleep 32\b", l)), None)
    if sleep is None:
        sys.exit("no `s_sleep 32` in the listing: not a resident instantiation?")
    at = next(n for n, b in enumerate(bl) if b["lo"] <= sleep < b["hi"])
    hdr = next(n for n in range(at, -1, -1) if bl[n]["is_header"])
    name = bl[hdr]["label"].lstrip(".L")
    loop = [n for n, b in enumerate(bl) if n == hdr or b["header"] == name]
    last = max(loop)
    parts = {"front": (bl[max(0, hdr - 6)]["lo"], bl[hdr]["lo"]), "look": (bl[hdr]["lo"], sleep + 1),
             "re-request": (sleep + 1, bl[last]["hi"]), "exit": (bl[last + 1]["lo"], bl[last + 1]["hi"])}
    print(f"{path}: gather loop {bl[hdr]['label']} .. {bl[last]['label']} (lines {bl[hdr]['lo'] + 1} - {bl[last]['hi']})")
    print(f"{'part':12s} " + " ".join(f"{k:>20s}" for k in COUNTED))
    for part, (lo, hi) in parts.items():
        c = count(lines, lo, hi)
        print(f"{part:12s} " + " ".join(f"{c[k]:20d}" for k in COUNTED))
    whole = "\n".join(lines)
    for op in ("v_max_f64", "v_mad_i64_i32", "v_lshl_add_u64"):
        print(f"{op:16s} {sum(1 for l in lines if l.split() and l.split()[0].startswith(op))}")
    for key in ("codeLenInByte", ".private_segment_fixed_size", ".sgpr_spill_count", ".vgpr_spill_count"):
        m = re.search(re.escape(key) + r"\D+(\d+)", whole)
        print(f"{key.lstrip('.'):28s} {m.group(1) if m else '?'}")
    # in-place loads: nothing names their registers before the wait written behind them
    in_asm, aimed, bad, n_loads = False, set(), [], 0
    for i, l in enumerate(lines):
        if "#ASMSTART" in l:
            in_asm = True
            continue
        if "#ASMEND" in l:
            in_asm = False
            continue
        t = l.split(";")[0].strip()
        if not t or t.endswith(":"):
            continue
        if in_asm and t.startswith("buffer_load_dwordx4"):
            m = re.match(r"buffer_load_dwordx4 v\[(\d+):(\d+)\]", t)
            aimed.update(range(int(m.group(1)), int(m.group(2)) + 1))
            n_loads += 1
        elif (in_asm and t.startswith("s_waitcnt vmcnt(0)")) or t.startswith("s_branch"):
            aimed.clear()  # (behind an unconditional branch the text is no longer the path: blocks moved out of line)
        elif aimed and not in_asm and regs(t) & aimed:
            bad.append((i + 1, t))
    print(f"in-place loads: {n_loads}; instructions that name a register between such a load and its wait: {len(bad)}")
    for i, t in bad:
        print(f"  line {i}: {t}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
