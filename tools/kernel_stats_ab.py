#!/usr/bin/env python3
"""tools/kernel_stats_ab.py PARENT_DIR LABEL=DIR [LABEL=DIR ...]: per-kernel comparison of rocprofv3 --kernel-trace --stats runs, the
layout of profiles/r30/lean_kernel_stats.txt.  Every DIR holds one run's *kernel_stats.csv (searched recursively), or those of several
runs of one library, which are pooled.  Per kernel:
launches, the parent's average (standard deviation) over the launches in microseconds, the other run's, the difference, the margin
3 x (parent's StdDev) / sqrt(launches), the verdict.  Kernels below --min-share (default 0.002) of the parent run's kernel time are
left out.

The primary stage's instances that regenerate directions carry other template arguments than the parent's -- shade_miss_kernel /
shade_hit_kernel <.., 3> for <.., 0>, traceq4_kernel<.., 3> for <.., 2> -- and are compared with the instance they replace; the row
shows both names."""
import csv, glob, math, os, re, sys


def load(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not f:
        sys.exit("no *kernel_stats.csv under " + d)
    # several runs under one DIR are pooled: launches and totals add up, the deviation is that of all launches about their common mean
    runs = {}
    for path in sorted(f):
        for r in csv.DictReader(open(path)):
            name = re.sub(r"^void ", "", r["Name"]).replace("ezd::", "")
            runs.setdefault(name, []).append((int(r["Calls"]), float(r["AverageNs"]) / 1e3, float(r["StdDev"]) / 1e3, float(r["TotalDurationNs"]) / 1e3))
    out = {}
    for name, rs in runs.items():
        n = sum(r[0] for r in rs)
        mean = sum(r[0] * r[1] for r in rs) / n
        ss = sum((r[0] - 1) * r[2] ** 2 + r[0] * (r[1] - mean) ** 2 for r in rs)
        out[name] = (n, mean, math.sqrt(ss / (n - 1)) if n > 1 else 0.0, sum(r[3] for r in rs))
    return out


def replaced(name):
    """the parent's instance a regenerating instance stands in for"""
    m = re.match(r"(shade_(?:miss|hit)_kernel<\d+, false, )3(>.*)", name)
    if m:
        return m.group(1) + "0" + m.group(2)
    m = re.match(r"(traceq4_kernel<\d, true, false, 2, true, false, false, )3(>.*)", name)
    if m:
        return m.group(1) + "2" + m.group(2)
    return name


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    min_share = 0.002
    for a in sys.argv[1:]:
        if a.startswith("--min-share="):
            min_share = float(a.split("=")[1])
    parent = load(args[0])
    run_total = sum(v[3] for v in parent.values())
    print("# kernel | launches | parent avg (StdDev) | other avg (StdDev) | diff | margin | verdict")
    for spec in args[1:]:
        label, d = spec.split("=", 1)
        other = load(d)
        print("## " + label)
        for name, (calls, avg, sd, total) in sorted(other.items(), key=lambda kv: -kv[1][3]):
            pname = name if name in parent else replaced(name)  # (a parent from round 31 on has the regenerating instances itself)
            if pname not in parent or parent[pname][3] < min_share * run_total:
                continue
            pc, pavg, psd, _ = parent[pname]
            margin = 3.0 * psd / math.sqrt(pc)
            diff = avg - pavg
            verdict = "one launch" if pc == 1 else ("within" if abs(diff) <= margin else ("lower" if diff < 0 else "HIGHER"))
            shown = name if pname == name else "%s  [for %s]" % (name, pname.split("(")[0])
            print("%-96s %5d %10.1f (%8.1f) %10.1f (%8.1f) %+9.1f %8.1f  %s" % (shown, calls, pavg, psd, avg, sd, diff, margin, verdict))


if __name__ == "__main__":
    main()
