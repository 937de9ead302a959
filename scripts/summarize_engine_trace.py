"""Engine launches of a rocprofv3 --kernel-trace run of bench.py: per kernel of the split chain
engine (k_odom_roles / k_odom_items, and the paired k_odom_roles2 / k_odom_items2) the launches,
launches per step and durations, and the share of paired launches.

Usage: python scripts/summarize_engine_trace.py <trace_kernel_trace.csv> <steps run (warmup + timed)>
"""
import csv
import sys


def base(name):
    return name.replace("void ", "").split("(")[0].split("<")[0].split("::")[-1]


def main():
    path, steps = sys.argv[1], int(sys.argv[2])
    durs = {}
    for r in csv.DictReader(open(path)):
        k = base(r["Kernel_Name"])
        if k.startswith("k_odom_items") or k.startswith("k_odom_roles"):
            durs.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    print(f"# {path}: {steps} steps")
    print("# kernel  launches  per_step  mean_ms  min_ms  max_ms  sum_ms_per_step")
    for k in sorted(durs):
        d = durs[k]
        print(f"{k}  {len(d)}  {len(d) / steps:.2f}  {sum(d) / len(d):.2f}  {min(d):.2f}  {max(d):.2f}  {sum(d) / steps:.2f}")
    single = sum(len(v) for k, v in durs.items() if k.startswith("k_odom_items") and not k.startswith("k_odom_items2"))
    paired = len(durs.get("k_odom_items2", []))
    chains = single + 2 * paired
    print(f"# item launches per step {(single + paired) / steps:.2f}; paired launches {paired} of {single + paired} "
          f"({100.0 * paired / max(1, single + paired):.0f} %), serving {2 * paired} of {chains} chains")


if __name__ == "__main__":
    main()
