"""The MoE block's stylization launch, the folded text cross-attention and the FFN launch behind it in a rocprofv3 --kernel-trace
CSV (un-probed `bench.py --no-graph` steps), per time scale.  With the text epilogue the stylization launch is the TX form of
style_gemm_kernel (<.., 0, true>) and there is no sd_fold launch; without it (the parent, or knob 174) sd_fold_kernel sits between
the stylization launch (<.., 0>) and the FFN.  The FFN behind it is one fused_mlp_stream_kernel launch at the full scale and two
GEMM launches at the coarse scale.
    python tools/text_epilogue_launches.py <rocprofv3 output dir>"""
import collections, csv, glob, os, re, statistics, sys

d = sys.argv[1]
tr = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
rows = sorted(csv.DictReader(open(tr)), key=lambda r: int(r["Start_Timestamp"]))


def short(n):
    n = n.replace("void ", "").replace("mdm::(anonymous namespace)::", "").replace("mdm::", "")
    return re.sub(r"\(.*", "", n)


def us(r):
    return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3


def wgs(r):
    return int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"]))


agg = collections.defaultdict(list)
for i, r in enumerate(rows):
    n = short(r["Kernel_Name"])
    tx = re.match(r"style_gemm_kernel<H[BF], true, 2, 0, true>", n)
    if not (tx or n.startswith("sd_fold_kernel")) or i + 2 >= len(rows) or i == 0:
        continue
    ffn = short(rows[i + 1]["Kernel_Name"])
    scale = "full" if ffn.startswith("fused_mlp_stream_kernel") else "coarse"
    if tx:
        agg[(scale, "1 MoE stylization + text epilogue", n, wgs(r))].append(us(r))
    else:
        agg[(scale, "1 MoE stylization", short(rows[i - 1]["Kernel_Name"]), wgs(rows[i - 1]))].append(us(rows[i - 1]))
        agg[(scale, "2 sd_fold", n, wgs(r))].append(us(r))
    agg[(scale, "3 FFN behind it", ffn, wgs(rows[i + 1]))].append(us(rows[i + 1]))
    if scale == "coarse":
        agg[(scale, "4 FFN, second GEMM", short(rows[i + 2]["Kernel_Name"]), wgs(rows[i + 2]))].append(us(rows[i + 2]))
print(f"{'scale':7s} {'launch':34s} {'kernel':46s} {'wgs':>5s} {'calls':>6s} {'median_us':>10s} {'p25_us':>8s} {'p75_us':>8s} {'min_us':>8s} {'max_us':>8s}")
tot = collections.defaultdict(float)
for k in sorted(agg):
    v = sorted(agg[k])
    q = statistics.quantiles(v, n=4) if len(v) > 1 else [v[0]] * 3
    tot[k[0]] += statistics.median(v)
    print(f"{k[0]:7s} {k[1][2:]:34s} {k[2][:46]:46s} {k[3]:5d} {len(v):6d} {statistics.median(v):10.1f} {q[0]:8.1f} {q[2]:8.1f} {v[0]:8.1f} {v[-1]:8.1f}")
for s in sorted(tot):
    print(f"{s:7s} sum of the medians above: {tot[s]:.1f} us per layer")
