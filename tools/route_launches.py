"""Router-centred summary of a rocprofv3 --kernel-trace run of bench.py --no-graph: dispatches per forward, and per (kernel,
workgroups, predecessor) the launches around the MoE router."""
import csv, re, collections, sys, glob, os
d, nfwd = sys.argv[1], int(sys.argv[2])
tr = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
def short(n):
    n = n.replace('void ', '').replace('mdm::(anonymous namespace)::', '')
    return re.sub(r'\(.*', '', n)[:60]
rows = sorted(csv.DictReader(open(tr)), key=lambda r: int(r['Start_Timestamp']))
tot = sum(int(r['End_Timestamp']) - int(r['Start_Timestamp']) for r in rows)
print(f"{len(rows)} kernel dispatches, {tot/1e6:.2f} ms of kernel time over {nfwd} sampling steps -> {len(rows)/nfwd:.1f} dispatches, {tot/1e6/nfwd:.3f} ms per step")
agg = collections.defaultdict(list)
prev = ''
for r in rows:
    n = short(r['Kernel_Name'])
    wg = int(r['Grid_Size_X']) // max(int(r['Workgroup_Size_X']), 1)
    key = (n, wg)
    if n.startswith('style_gemm_kernel'): key = (n + ' after ' + prev.split('<')[0], wg)
    if n.startswith(('style_gemm_kernel', 'moe_')): agg[key].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    prev = n
print(f"{'kernel':88s} {'wgs':>5s} {'calls':>6s} {'/step':>6s} {'avg_us':>8s} {'med_us':>8s} {'us/step':>8s}")
for k, v in sorted(agg.items()):
    v.sort()
    print(f"{k[0]:88s} {k[1]:5d} {len(v):6d} {len(v)/nfwd:6.1f} {sum(v)/len(v):8.2f} {v[len(v)//2]:8.2f} {sum(v)/nfwd:8.1f}")
