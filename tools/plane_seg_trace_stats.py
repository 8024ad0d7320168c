"""Sums the per-dispatch rows of `rocprofv3 --kernel-trace --output-format csv -- python tools/plane_seg_time.py --repeats R` per
kernel, the two count kernels per configuration as well: the tool's dispatches come in a fixed order (for every size: 1 + R plane
counts and 1 + R pair counts per model count, then 1 + R segmentations at each of two max_iterations), so the k-th dispatch of
k_plane_count or k_sac_count in time order names its configuration.  Writes what profiles/plane_seg_kernel_stats.csv holds.

    python tools/plane_seg_trace_stats.py <kernel_trace.csv> <out.csv> [--sizes 307200,1000000] [--models 1024,4096] [--repeats 5]
"""
import argparse
import csv
import re


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("out")
    ap.add_argument("--sizes", default="307200,1000000")
    ap.add_argument("--models", default="1024,4096")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    sizes, models, calls = a.sizes.split(","), a.models.split(","), 1 + a.repeats
    plane_labels, pair_labels = [], []
    for n in sizes:
        for H in models:
            plane_labels += ["n %s, H %s" % (n, H)] * calls
            pair_labels += ["n %s, H %s" % (n, H)] * calls
        plane_labels += ["n %s, in plane_segment" % n] * (2 * calls)
    rows = sorted(csv.DictReader(open(a.trace)), key=lambda r: int(r["Start_Timestamp"]))
    seen, stats = {}, {}
    for r in rows:
        name = re.sub(r"^(void )?(rsreg::)?", "", r["Kernel_Name"]).split("(")[0].split("<")[0]
        k = seen.get(name, 0)
        seen[name] = k + 1
        if name == "k_plane_count":
            name += " [%s]" % plane_labels[k]
        elif name == "k_sac_count":
            name += " [%s]" % pair_labels[k]
        stats.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    assert seen.get("k_plane_count", 0) == len(plane_labels) and seen.get("k_sac_count", 0) == len(pair_labels), seen
    total = sum(sum(v) for v in stats.values())
    with open(a.out, "w", newline="") as f:
        w = csv.writer(f, quoting=csv.QUOTE_NONNUMERIC)
        w.writerow(["Name", "Calls", "TotalDurationUs", "AverageUs", "MinUs", "MaxUs", "Percentage"])
        for name, v in sorted(stats.items(), key=lambda kv: -sum(kv[1])):
            w.writerow([name, len(v), round(sum(v), 1), round(sum(v) / len(v), 1), round(min(v), 1), round(max(v), 1), round(100 * sum(v) / total, 2)])


if __name__ == "__main__":
    main()
