"""Diagnostics: registers, spills, scratch and static LDS of every k_robot_sweep instantiation, every form of the resident ones
included (feat: 0 lean, 2 with prior updates, 3 full, 7 masked: full with the kinds per robot group) (hipcc -Rpass-analysis=kernel-resource-usage).
usage: python tools/kernel_resources.py [extra hipcc flags ...]"""
import os, re, subprocess, sys
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = os.path.join(ROOT, "magics_amd", "csrc", "mgx_sweep_inst.hip")


def remarks(fk):
    f, k, ft = fk
    return subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", "-ffp-contract=off", f"-DMGX_FLAVOR={f}", f"-DMGX_KSET={k}", f"-DMGX_FEAT={ft}",
                           "-Rpass-analysis=kernel-resource-usage", *sys.argv[1:], src, "-o", f"/tmp/_kernel_resources_{f}{k}{ft}.o"],
                          capture_output=True, text=True).stderr


with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 2)) as ex:
    out = "\n".join(ex.map(remarks, [(f, k, ft) for f in range(3) for k in range(3) for ft in (((7, 3, 2, 0) if f == 1 else (3, 2, 0)) if f else (3,))]))
cur, rows = None, {}
for line in out.splitlines():
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = m.group(1)
        rows[cur] = {}
        continue
    m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
    if m and cur:
        rows[cur][m.group(1).strip()] = int(m.group(2))
print(f"{'kernel':52s} {'VGPR':>5s} {'AGPR':>5s} {'SGPR':>5s} {'v-spill':>8s} {'s-spill':>8s} {'scratch':>8s} {'LDS':>6s} {'occ':>4s}")
table = []
for name, r in rows.items():
    m = re.match(r"_ZN3mgx13k_robot_sweepILi(n?\d+)ELi(\d)ELb(\d)ELb(\d)ELj(\d)EE", name)
    if not m:
        continue
    k = int(m.group(1).replace("n", "-"))
    table.append((k, int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5)), r))
for k, irm, per, sh, ft, r in sorted(table, key=lambda t: (t[0] <= 0, t[0], t[1], t[2], t[3], -t[4])):
    label = f"k_robot_sweep<{k:>3d}, {irm}, {'true ' if per else 'false'}{', shard' if sh else ''}{f', feat {ft}' if per else ''}>"
    print(f"{label:52s} {r.get('VGPRs', 0):5d} {r.get('AGPRs', 0):5d} {r.get('TotalSGPRs', 0):5d} "
          f"{r.get('VGPRs Spill', 0):8d} {r.get('SGPRs Spill', 0):8d} {r.get('ScratchSize', 0):8d} {r.get('LDS Size', 0):6d} {r.get('Occupancy', 0):4d}")
