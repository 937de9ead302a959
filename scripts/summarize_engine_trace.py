"""Engine launches of a rocprofv3 --kernel-trace run of bench.py: per kernel of the split chain
engine (k_odom_roles / k_odom_items, and the paired k_odom_roles2 / k_odom_items2) the launches,
launches per step and durations, the share of paired launches and the engine slot-ms per step.

With segments (lislam_set_engine_segment) a chain is several launches.  The trace does not name a
launch's chains, so they are linked by time: a launch continues the chains whose last segment ended
most recently before it started (one for k_odom_items, up to two for k_odom_items2) and opens new
chains for the rest; a chain is complete after `segments per chain` launches (ceil(pairs / L); 1 =
whole chains, the default).  From the links: the chains' spans from their first segment's start to
their last one's end, and the gap between a chain's consecutive segments (what a boundary costs).

Usage: python scripts/summarize_engine_trace.py <trace_kernel_trace.csv> <steps run (warmup + timed)> [segments per chain]
"""
import csv
import sys


def base(name):
    return name.replace("void ", "").split("(")[0].split("<")[0].split("::")[-1]


def link_chains(launches, per_chain):
    """launches: (start_ms, end_ms, chains carried) of the item kernels.  Returns the complete chains
    as (first start, last end, segments, paired segments) and every gap between linked segments."""
    open_chains, done, gaps = [], [], []
    for start, end, cap in sorted(launches):
        cont = sorted((c for c in open_chains if c["end"] <= start), key=lambda c: -c["end"])[:cap]
        for c in cont:
            gaps.append(start - c["end"])
            c["end"], c["segs"], c["paired"] = end, c["segs"] + 1, c["paired"] + (cap == 2)
        for _ in range(cap - len(cont)):
            open_chains.append({"start": start, "end": end, "segs": 1, "paired": int(cap == 2)})
        for c in [c for c in open_chains if c["segs"] >= per_chain]:
            open_chains.remove(c)
            done.append((c["start"], c["end"], c["segs"], c["paired"]))
    return done, gaps, len(open_chains)


def main():
    path, steps = sys.argv[1], int(sys.argv[2])
    per_chain = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    durs, launches = {}, []
    for r in csv.DictReader(open(path)):
        k = base(r["Kernel_Name"])
        if k.startswith("k_odom_items") or k.startswith("k_odom_roles"):
            t0, t1 = int(r["Start_Timestamp"]) / 1e6, int(r["End_Timestamp"]) / 1e6
            durs.setdefault(k, []).append(t1 - t0)
            if k.startswith("k_odom_items"):
                launches.append((t0, t1, 2 if k.startswith("k_odom_items2") else 1))
    print(f"# {path}: {steps} steps")
    print("# kernel  launches  per_step  mean_ms  min_ms  max_ms  sum_ms_per_step")
    for k in sorted(durs):
        d = durs[k]
        print(f"{k}  {len(d)}  {len(d) / steps:.2f}  {sum(d) / len(d):.2f}  {min(d):.2f}  {max(d):.2f}  {sum(d) / steps:.2f}")
    single = sum(len(v) for k, v in durs.items() if k.startswith("k_odom_items") and not k.startswith("k_odom_items2"))
    paired = len(durs.get("k_odom_items2", []))
    chains = single + 2 * paired
    slot_ms = sum(sum(v) for k, v in durs.items() if k.startswith("k_odom_items"))
    print(f"# item launches per step {(single + paired) / steps:.2f}; paired launches {paired} of {single + paired} "
          f"({100.0 * paired / max(1, single + paired):.0f} %), serving {2 * paired} of {chains} chains"
          f"{'' if per_chain == 1 else ' (chain-segments)'}; engine slot-ms per step {slot_ms / steps:.2f}")
    if per_chain > 1:
        done, gaps, left = link_chains(launches, per_chain)
        spans = [e - s for s, e, _, _ in done]
        segs = sum(n for _, _, n, _ in done)
        shared = sum(p for _, _, _, p in done)
        print(f"# segments per chain {per_chain}: {len(done)} complete chains ({left} left open), {segs} chain-segments, "
              f"{shared} of them in a paired launch ({100.0 * shared / max(1, segs):.0f} %)")
        if spans:
            print(f"# chain span, first segment's start to last one's end: mean {sum(spans) / len(spans):.2f} ms, "
                  f"min {min(spans):.2f}, max {max(spans):.2f}")
        if gaps:
            g = sorted(gaps)
            print(f"# gap between a chain's consecutive segments: median {g[len(g) // 2]:.3f} ms, mean {sum(g) / len(g):.3f}, "
                  f"p90 {g[len(g) * 9 // 10]:.3f}, max {g[-1]:.3f}")


if __name__ == "__main__":
    main()
