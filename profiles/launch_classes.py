"""Per-kernel launch counts by duration class from a rocprofv3 kernel trace
(the `*_launches_si1m.txt` files of this directory):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- \\
        python bench.py --steps 2 --warmup 1
    python profiles/launch_classes.py DIR > NAME_launches.txt
A launch's class is its duration rounded to 0.1 ms below 2 ms and to 1 ms
above.  The kernel trace itself (one row per launch) is not committed."""
import collections
import csv
import glob
import os
import sys

PATTERNS = ["Cijk_Alik_Bljk", "CUDAFunctor_add", "k_gather_rows_v4",
            "k_edge_mlp_bwd", "k_gated_mlp_tail_bwd", "k_gated_mlp_tail_fwd",
            "k_gated_mlp_64", "k_edge_mlp_64x128", "k_seg_sum"]


def main(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"),
                  recursive=True)[0]
    by = collections.defaultdict(list)
    with open(f) as fh:
        for r in csv.DictReader(fh):
            by[r["Kernel_Name"]].append(
                (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    n = sum(len(v) for v in by.values())
    tot = sum(sum(v) for v in by.values())
    print(f"# {os.path.basename(f)}: {n} launches, {tot:.1f} ms of kernels")
    ranked = sorted(by.items(), key=lambda kv: -sum(kv[1]))
    for name, v in ranked:
        if not any(p in name for p in PATTERNS):
            continue
        v2 = sorted(v)
        cls = collections.Counter(round(x, 1) if x < 2 else round(x)
                                  for x in v)
        top = ", ".join(f"{k}ms x{c}" for k, c in sorted(
            cls.items(), key=lambda kc: -kc[0] * kc[1])[:8])
        print(f"{name[:110]}\n   n={len(v)} total={sum(v):.1f} ms "
              f"max={v2[-1]:.2f} median={v2[len(v2) // 2]:.2f} | {top}")
    print("# top 25 by total")
    for name, v in ranked[:25]:
        print(f"{sum(v):9.1f} ms  n={len(v):5d}  max={max(v):7.2f}  "
              f"{name[:100]}")


if __name__ == "__main__":
    main(sys.argv[1])
