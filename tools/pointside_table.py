"""Per-launch table of the point-side kernels (thin fp32 linears, projection MLP, their reductions and the GNO fix-ups) from a
rocprofv3 kernel trace of eager bench steps.

    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python3 bench.py --steps 5 --warmup 2 --no-graph --no-secondary
    python3 tools/pointside_table.py DIR OUT.txt [SITES.txt]

A step is cut at every `k_mlp2_fwd` launch (the forward's last point-side kernel; the workload must run the fused projection MLP),
so a row's position is its place in "backward of a step, then the next forward"; the steps with the most common launch sequence are
averaged.  SITES.txt (optional, written by hand from the order of the step): lines `<pos> <call site, shape>` appended to the row."""
import csv
import glob
import re
import sys
from collections import Counter, defaultdict

PAT = re.compile(r"k_gemm<4|k_splitk_reduce|k_colsum|k_act_bwd|k_transpose_w|k_mlp2|k_scale_by_inv_deg|k_segment_fixup|k_rowlin|k_reduce_multi")


def short(name):
    name = re.sub(r"^void ", "", name).replace("(anonymous namespace)::", "")
    return re.sub(r"\(.*$", "", name)


def main(argv):
    if len(argv) not in (3, 4):
        sys.exit(__doc__)
    traces = glob.glob(argv[1] + "/**/*kernel_trace.csv", recursive=True)
    if not traces:
        sys.exit(f"no *kernel_trace.csv under {argv[1]}")
    sites = {}
    if len(argv) == 4:
        for line in open(argv[3]):
            pos, _, text = line.strip().partition(" ")
            if pos.isdigit():
                sites[int(pos)] = text
    rows = []
    with open(traces[0]) as fh:
        for r in csv.DictReader(fh):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Grid_Size_X", r.get("Grid_Size", "")),
                         r.get("Workgroup_Size_X", r.get("Workgroup_Size", ""))))
    rows.sort()
    cycles, cur = [], []
    for s, e, n, g, w in rows:
        if not PAT.search(n):
            continue
        sn = short(n)
        if "k_mlp2_fwd" in sn and cur:
            cycles.append(cur)
            cur = []
        cur.append((sn, g, w, (e - s) / 1000.0))
    if not cycles:
        sys.exit("no k_mlp2_fwd launch in the trace: nothing to cut the steps at")
    sig = lambda c: tuple((x[0], x[1]) for x in c)
    common = Counter(sig(c) for c in cycles).most_common(1)[0][0]
    good = [c for c in cycles if sig(c) == common]
    with open(argv[2], "w") as o:
        o.write(f"# {len(good)} steps averaged (cycle = k_mlp2_fwd .. next k_mlp2_fwd: backward of a step, then the next forward)\n")
        o.write("# pos kernel grid(threads) wg mean_us min_us max_us | call site, shape\n")
        tot, cnt, total = defaultdict(float), defaultdict(int), 0.0
        for i in range(len(good[0])):
            v = [c[i][3] for c in good]
            n, g, w, _ = good[0][i]
            m = sum(v) / len(v)
            o.write(f"{i:3d} {n} {g} {w} {m:.1f} {min(v):.1f} {max(v):.1f}{' | ' + sites[i] if i in sites else ''}\n")
            tot[n] += m
            cnt[n] += 1
            total += m
        o.write("# per kernel: launches, us per step\n")
        for n in sorted(tot, key=lambda k: -tot[k]):
            o.write(f"# {n} {cnt[n]} {tot[n]:.1f}\n")
        o.write(f"# sum {total:.1f} us per step\n")


if __name__ == "__main__":
    main(sys.argv)
