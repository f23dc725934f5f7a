"""The dual block's skip projection and its two pair + tail launches in a rocprofv3 --kernel-trace CSV (un-probed
`bench.py --no-graph` steps), per time scale: the skip GEMM launches (gemm_bf16_kernel<.., ACT_GELU> on 392 blocks), the first
(local Performer) and the second (global) pair + tail launch of every block.  Within a scale the pair + tail launches alternate
local, global; with riders the local one is pair_tail_rider_kernel.
    python tools/skip_rider_launches.py <rocprofv3 output dir>"""
import collections, csv, glob, os, re, statistics, sys

d = sys.argv[1]
tr = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
rows = sorted(csv.DictReader(open(tr)), key=lambda r: int(r["Start_Timestamp"]))
agg = collections.defaultdict(list)
seen = collections.Counter()  # pair + tail launches so far, per scale
for r in rows:
    n = r["Kernel_Name"]
    us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    wgs = int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"]))
    m = re.search(r"fused_mlp_stream_kernel<mdm::H[BF], (\d), 4, 512, 1>", n) or re.search(r"pair_tail_rider_kernel<mdm::H[BF], (\d)>", n)
    if m:
        scale = "coarse" if m.group(1) == "2" else "full"
        which = "local " if seen[scale] % 2 == 0 else "global"
        seen[scale] += 1
        agg[(scale, f"pair + tail, {which}", "riders" if "rider" in n else "plain", wgs)].append(us)
        continue
    m = re.search(r"gemm_bf16_kernel<mdm::H[BF], (\d+), 64, \d, 1>", n)
    if m and wgs == 392:
        agg[("coarse" if m.group(1) == "64" else "full", "skip GEMM launch  ", "", wgs)].append(us)
print(f"{'scale':7s} {'launch':20s} {'form':7s} {'wgs':>4s} {'calls':>6s} {'median_us':>10s} {'min_us':>8s} {'max_us':>8s}")
for k in sorted(agg):
    v = agg[k]
    print(f"{k[0]:7s} {k[1]:20s} {k[2]:7s} {k[3]:4d} {len(v):6d} {statistics.median(v):10.1f} {min(v):8.1f} {max(v):8.1f}")
