"""Mean duration per (kernel, grid) from a rocprofv3 --kernel-trace CSV directory: the same kernel launched on two grids (the critics' and the
actor's wgrad launch) is two populations, which --stats' per-name mean hides.   python3 tools/kernel_by_grid.py <trace dir> [name filter]"""
import collections
import csv
import glob
import re
import statistics
import sys


def short(n):
    n = re.sub(r"\(anonymous namespace\)::", "", n)
    n = re.sub(r"^void ", "", n)
    return n.split("(")[0][:60]


def main():
    root, pat = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "")
    rows = []
    for f in glob.glob(root + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            wg = [max(1, int(r.get("Workgroup_Size_" + a, 1) or 1)) for a in "XYZ"]
            grid = tuple(int(r.get("Grid_Size_" + a, 0) or 0) // w for a, w in zip("XYZ", wg))  # rocprofv3 counts work-items: -> workgroups
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]), grid))
    rows.sort()
    rows = rows[len(rows) // 3:]  # steady state
    dur = collections.defaultdict(list)
    for s, e, n, g in rows:
        if pat in n:
            dur[(n, g)].append((e - s) / 1e3)
    print(f"{'kernel':62s} {'grid (workgroups)':>18s} {'calls':>7s} {'mean us':>8s} {'median':>8s} {'sd':>6s}")
    for (n, g), d in sorted(dur.items(), key=lambda kv: -sum(kv[1])):
        print(f"{n:62s} {'x'.join(map(str, g)):>18s} {len(d):7d} {statistics.fmean(d):8.2f} {statistics.median(d):8.2f} {statistics.pstdev(d):6.2f}")


if __name__ == "__main__":
    main()
