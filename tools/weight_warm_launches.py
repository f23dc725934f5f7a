"""Hosts and consumers of the weight warming (csrc/warm.h) in a rocprofv3 --kernel-trace CSV of un-probed `bench.py --no-graph`
steps: medians per (kernel, scale, grid).  The scale comes from the kernel's template arguments where they carry it (row tiles of
the attention core: 7 coarse / 13 full; of the pair + tail launch: 2 / 4; of the query core: its row-tile count), otherwise the
launches of one (kernel, grid) are listed together.  Within a scale the attention cores and the pair + tail launches alternate
local, global.
    python tools/weight_warm_launches.py <rocprofv3 output dir>"""
import collections, csv, glob, os, re, statistics, sys

d = sys.argv[1]
tr = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
rows = sorted(csv.DictReader(open(tr)), key=lambda r: int(r["Start_Timestamp"]))
WATCH = ("perf_attn_kernel", "fused_mlp_stream_kernel", "pair_tail_rider_kernel", "lin_xattn_q_kernel", "style_gemm_kernel",
         "ln_chain_kernel", "sd_fold_kernel")


def short(n):
    n = n.replace("void ", "").replace("mdm::(anonymous namespace)::", "").replace("mdm::", "")
    return re.sub(r"\(.*", "", n)


agg = collections.defaultdict(list)
seen = collections.Counter()
for r in rows:
    n = short(r["Kernel_Name"])
    if not n.startswith(WATCH):
        continue
    us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    wgs = int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"]))
    scale, which = "-", ""
    m = re.match(r"perf_attn_kernel<H[BF], (\d+)>", n)
    if m:
        scale = "coarse" if m.group(1) == "7" else "full"
    m2 = re.match(r"fused_mlp_stream_kernel<H[BF], (\d), 4, 512, 1>", n) or re.match(r"pair_tail_rider_kernel<H[BF], (\d)>", n)
    if m2:
        scale = "coarse" if m2.group(1) == "2" else "full"
    if m or m2:
        k = ("attn" if m else "pair", scale)
        which = "local" if seen[k] % 2 == 0 else "global"
        seen[k] += 1
    agg[(n, scale, which, wgs)].append(us)
print(f"{'kernel':52s} {'scale':6s} {'which':6s} {'wgs':>5s} {'calls':>6s} {'median_us':>10s} {'p25_us':>8s} {'p75_us':>8s} {'min_us':>8s} {'max_us':>8s}")
for k in sorted(agg):
    v = sorted(agg[k])
    q = statistics.quantiles(v, n=4) if len(v) > 1 else [v[0]] * 3
    print(f"{k[0][:52]:52s} {k[1]:6s} {k[2]:6s} {k[3]:5d} {len(v):6d} {statistics.median(v):10.1f} {q[0]:8.1f} {q[2]:8.1f} {v[0]:8.1f} {v[-1]:8.1f}")
