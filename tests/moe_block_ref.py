"""Plain restatement of the MoE inference block (MoEMultiBranchFFN + StylizationBlock + residual) for the block tests, in any
dtype and on any device: two branches of LayerNorm -> gate -> softmax -> top-2 (lowest index first), the serial expert loop with
probabilities that are NOT renormalised, the mean of the branches, the stylization on given (scale | shift) rows, the residual.

Run in fp64 it is the reference of tests/test_moe_block_gpu.py; run in fp32 it equals oracle/denoiser_ref.py:moe_ffn, which the
reference-generated goldens vouch for (tests/test_moe_block_ref.py).  No fixtures, no GPU code, nothing from the package but the
seeded weight builders.

The last section restates the fp8 mode's block (precision 5) STAGE BY STAGE for tests/test_fp8_block_gpu.py: every stage in fp64 on
the operands the stage before it actually left (e4m3 rows and scales, the e4m3 hidden layer, the fp16 expert outputs), with
bounds that are rounding properties of e4m3 / fp16 or gates the project already uses -- no end-to-end tolerance that would
depend on how e4m3 near-ties resolve."""
import importlib
from collections import namedtuple

import torch
import torch.nn.functional as F

PRE = "decoder_blocks_low.0.module.ffn"


def _pkg(sub):
    return importlib.import_module("motiondiffusion-moe_amd." + sub)


def block_state(D, H, Fd, E, seed, num_frames=60, experts=True):
    """The block's sub-state {key: fp32 tensor}: the `decoder_blocks_low.0.module.ffn.*` keys of a one-layer model of this
    width, filled by the seeded builder (experts=False: without the expert matrices, for the router alone)."""
    keys = _pkg("layout").state_dict_layout(8, num_frames=num_frames, latent_dim=D, ff_size=Fd, num_layers=1, num_heads=H,
                                            text_latent_dim=64, moe_num_experts=E, model_size="small")
    return _pkg("synth").synth_state_dict([(k, s) for k, s in keys if k.startswith(PRE + ".") and (experts or ".experts." not in k)], seed)


def block_inputs(B, S, D, seed):
    """h (B, S, D) rows, the block's (scale | shift) rows (B, 2D), ragged lengths (B,)."""
    synth = _pkg("synth")
    h = synth.uniform_pm1((B, S, D), "moeblk.h", seed) * 1.5
    sc = synth.uniform_pm1((B, 2 * D), "moeblk.sc", seed) * 0.5
    length = torch.tensor(([S, max(1, S - 13)] + [S] * B)[:B])
    return h, sc, length


def _lin(x, sd, p):
    return F.linear(x, sd[p + ".weight"], sd[p + ".bias"])


def _ln(x, sd, p):
    w = sd[p + ".weight"]
    return F.layer_norm(x, (w.shape[0],), w, sd[p + ".bias"], 1e-5)


def cast_state(sd, dtype, device="cpu"):
    return {k: v.to(device=device, dtype=dtype) for k, v in sd.items()}


def top2_lowest_index_first(probs):
    """(values (M, 2), indices (M, 2)): the largest entry, then the largest of the rest; the lowest index wins every tie."""
    E = probs.shape[1]
    ar = torch.arange(E, device=probs.device)
    v1 = probs.max(dim=1, keepdim=True).values
    i1 = torch.where(probs == v1, ar, E).min(dim=1).values
    rest = probs.masked_fill(ar[None] == i1[:, None], -1.0)
    v2 = rest.max(dim=1, keepdim=True).values
    i2 = torch.where(rest == v2, ar, E).min(dim=1).values
    return torch.cat([v1, v2], 1), torch.stack([i1, i2], 1)


def gate_logits(x, sd, br, pre=PRE):
    """(M, E) gate logits of branch br for rows x (.., D); x and sd share dtype and device."""
    D = x.shape[-1]
    return _lin(_ln(x, sd, f"{pre}.branches.{br}.layernorm").reshape(-1, D), sd, f"{pre}.branches.{br}.moe.gate")


def switch_moe(h, sd, p, E, forced=None):
    logits = _lin(h, sd, p + ".gate")
    probs = F.softmax(logits, dim=1)
    if forced is None:
        vals, idx = top2_lowest_index_first(probs)
    else:
        idx = forced.to(device=h.device, dtype=torch.int64)
        vals = probs.gather(1, idx)
    out = torch.zeros_like(h)
    usage = torch.zeros(E, dtype=h.dtype, device=h.device)
    imp = torch.zeros(E, dtype=h.dtype, device=h.device)
    for e in range(E):
        hit = idx == e
        rows = hit.any(dim=1)
        usage[e] = (idx[:, 0] == e).sum()
        if not bool(rows.any()):
            continue
        ye = _lin(F.gelu(_lin(h[rows], sd, f"{p}.experts.{e}.0")), sd, f"{p}.experts.{e}.2")
        pe = (vals * hit)[rows].sum(dim=1, keepdim=True)  # a token routed twice to e carries both probabilities
        out[rows] += pe * ye
        imp[e] = pe.sum()
    return out, dict(logits=logits, idx=idx, vals=vals, usage=usage, importance=imp)


def moe_block(x, sc, sd, E, forced=None, pre=PRE):
    """x (B, S, D), sc (B, 2D), sd in x's dtype on x's device; forced: None or (2, B*S, 2) indices.
    Returns (out (B, S, D), [per-branch dict(logits, idx, vals, usage, importance)])."""
    B, S, D = x.shape
    acc, info = 0, []
    for br in range(2):
        h = _ln(x, sd, f"{pre}.branches.{br}.layernorm").reshape(-1, D)
        o, tr = switch_moe(h, sd, f"{pre}.branches.{br}.moe", E, None if forced is None else forced[br])
        info.append(tr)
        acc = acc + o.view(B, S, D)
    return block_tail(x, acc / 2, sc, sd, pre), info


def block_tail(x, acc, sc, sd, pre=PRE):
    """The block behind the experts: acc (B, S, D) is the mean of the two branches; stylization on sc's (scale | shift), residual."""
    D = x.shape[-1]
    scale, shift = sc[:, None, :D], sc[:, None, D:]
    y = _ln(acc, sd, pre + ".proj_out.norm") * (1 + scale) + shift
    return x + _lin(F.silu(y), sd, pre + ".proj_out.out_layers.2")


def top3_gap(logits):
    """min(l1 - l2, l2 - l3) per row of (M, E) logits; l1 - l2 at E = 2."""
    t = logits.topk(min(3, logits.shape[1]), dim=1).values
    g = t[:, 0] - t[:, 1]
    return g if t.shape[1] < 3 else torch.minimum(g, t[:, 1] - t[:, 2])


def routing_margin(x32, sd32, sd64, br):
    """8 x max |fp32 restatement's logits - fp64 logits| of branch br (CPU tensors): what fp32 arithmetic in another order of
    summation may not tell apart.  Returns (margin, fp64 logits (M, E))."""
    l32 = gate_logits(x32, sd32, br).double()
    l64 = gate_logits(x32.double(), sd64, br)
    return 8.0 * float((l32 - l64).abs().max()), l64


# ---------------------------------------------------------------------------------------------------------------------
# the fp8 mode's block (precision 5), stage by stage
# ---------------------------------------------------------------------------------------------------------------------
def _e4m3_table():
    t = torch.empty(256, dtype=torch.float64)
    for b in range(256):
        e, m = (b >> 3) & 15, b & 7
        v = float("nan") if (e == 15 and m == 7) else (m * 2.0 ** -9 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7))
        t[b] = -v if b & 128 else v
    return t


E4M3 = _e4m3_table()


def e4m3_decode(b):
    """fp64 values of OCP e4m3 ("fn": no infinity) bytes: 4 exponent bits of bias 7, 3 mantissa bits, subnormals m * 2^-9, the
    largest magnitude 448; 0x7F and 0xFF are the two NaNs."""
    assert b.dtype == torch.uint8
    return E4M3.to(b.device)[b.long()]


def e4m3_nan_bytes(b):
    return int(((b & 0x7F) == 0x7F).sum())


def e4m3_step(v):
    """Spacing of the e4m3 values around v: 2 ** (max(floor(log2 |v|), -6) - 3), and 2^-9 at 0.  Round-to-nearest lands within half
    of it for |v| <= 448."""
    v = v.abs().double()
    _, ex = torch.frexp(v)  # |v| = m * 2^ex with m in [0.5, 1): floor(log2 |v|) = ex - 1
    fl = torch.where(v > 0, ex - 1, torch.full_like(ex, -6)).clamp_min(-6)
    return torch.ldexp(torch.ones_like(v), fl - 3)


def quantize_rows_e4m3(w):
    """torch's e4m3 conversion of fp32 rows under scale = amax / 448 per row (1 for an all-zero row), in the operation order of the
    library's quantisers (scale = amax * fp32(1 / 448), bytes = nearest-even(w * (1 / scale))): (bytes, scales)."""
    w = w.float()
    amax = w.abs().amax(-1)
    s = torch.where(amax > 0, amax * torch.tensor(1.0 / 448.0, dtype=torch.float32, device=w.device), torch.ones_like(amax))
    return (w * (1.0 / s)[..., None]).to(torch.float8_e4m3fn).view(torch.uint8), s


def ln_margin(x32, sd32, sd64, pre=PRE):
    """e_LN: 8 x the largest |fp32 restatement - fp64| of the two branch LayerNorms over the case (CPU tensors) -- the construction
    of routing_margin: what fp32 arithmetic in another order may not tell apart."""
    return 8.0 * max(float((_ln(x32, sd32, f"{pre}.branches.{br}.layernorm").double()
                            - _ln(x32.double(), sd64, f"{pre}.branches.{br}.layernorm")).abs().max()) for br in range(2))


Check = namedtuple("Check", "stage what ok worst")  # worst: the largest err / bound (or a count of offenders)


def _within(stage, what, err, bound):
    return Check(stage, what, bool((err <= bound).all()), float((err / bound).max()) if err.numel() else 0.0)


def failed_stages(checks):
    return sorted({c.stage for c in checks if not c.ok})


def fp8_block_stages(x, sc, sd64, E, e_ln, dev, wq, pre=PRE):
    """The fp8 mode's MoE block stage by stage, each stage in fp64 on what the stage before it left.
    x (B, S, D), sc (B, 2D), sd64: fp64 on one device (the buffers are moved there).  e_ln: ln_margin of the case.
    dev, the block's buffers after the run: x8 (2, M, D) uint8 e4m3 rows and s (2, M) fp32 their scales (router); perm (4M), goff
    (2E + 1), pos4 (M, 4), rowscale (4M) (the slab assignment, verified by the caller); hid (4M, F) uint8; y2 (4M, D) fp16;
    out (B, S, D) fp32.  wq: w1q (2E, F, D) / w2q (2E, D, F) uint8 and w1s (2E, F) / w2s (2E, D) fp32, the expert weights'
    e4m3 images and channel scales.  Rows of hid and y2 at or past goff[2E] enter no check.
    Returns ([Check], dict(v64, y64, want)): the stages' wanted values, for the caller's own figures."""
    B, S, D = x.shape
    M, two = B * S, torch.tensor(2.0, dtype=torch.float64)
    d = {k: v.to(x.device) for k, v in dev.items()}
    wq = {k: v.to(x.device) for k, v in wq.items()}
    checks = []
    # stage 1: the router's rows and scales against the fp64 LayerNorm of each branch
    h64 = torch.stack([_ln(x, sd64, f"{pre}.branches.{br}.layernorm").reshape(M, D) for br in range(2)])
    s = d["s"].double()
    a = e4m3_decode(d["x8"]) * s[..., None]
    checks.append(_within(1, "row scales", (s - h64.abs().amax(-1) / 448).abs(), two ** -21 * s + e_ln / 448))
    checks.append(_within(1, "rows", (a - h64).abs(), s[..., None] * e4m3_step(h64.abs() / s[..., None] + e_ln / s[..., None]) / 2 + e_ln))
    checks.append(Check(1, "no NaN byte", e4m3_nan_bytes(d["x8"]) == 0, float(e4m3_nan_bytes(d["x8"]))))
    top = e4m3_decode(d["x8"] & 0x7F).amax(-1)
    checks.append(Check(1, "every row's largest magnitude is 448", bool((top == 448).all()), float((top != 448).sum())))
    # stages 2 and 3: each expert GEMM on the device's own operands, per slab of goff
    perm, goff = d["perm"].long(), d["goff"].long().tolist()
    n = goff[2 * E]
    rows = a.reshape(2 * M, D)[perm[:n]]
    hid = e4m3_decode(d["hid"][:n])
    rowscale = d["rowscale"][:n].double()
    v64 = torch.empty((n, hid.shape[1]), dtype=torch.float64, device=x.device)
    y64 = torch.empty((n, D), dtype=torch.float64, device=x.device)
    for g in range(2 * E):
        lo, hi = goff[g], goff[g + 1]
        if hi == lo:
            continue
        p = f"{pre}.branches.{g // E}.moe.experts.{g % E}"
        w1 = e4m3_decode(wq["w1q"][g]) * wq["w1s"][g].double()[:, None]
        v64[lo:hi] = 8 * F.gelu(rows[lo:hi] @ w1.T + sd64[p + ".0.bias"])
        w2 = e4m3_decode(wq["w2q"][g]) * wq["w2s"][g].double()[:, None]
        y64[lo:hi] = rowscale[lo:hi, None] * ((hid[lo:hi] / 8) @ w2.T + sd64[p + ".2.bias"])
    e = 2e-5 * v64.abs().max()
    checks.append(_within(2, "hidden layer", (hid - v64.clamp(-448, 448)).abs(), e4m3_step((v64.abs() + e).clamp_max(448)) / 2 + e))
    checks.append(Check(2, "no NaN byte", e4m3_nan_bytes(d["hid"][:n]) == 0, float(e4m3_nan_bytes(d["hid"][:n]))))
    checks.append(_within(3, "expert outputs", (d["y2"][:n].double() - y64).abs(), two ** -11 * y64.abs() + two ** -25 + 2e-5 * y64.abs().max()))
    # stage 4: mean over pos4, stylization, residual on the device's y2; the fp16 mode's code and its gate
    acc = 0.5 * d["y2"].double()[d["pos4"].long()].sum(1)
    want = block_tail(x, acc.view(B, S, D), sc, sd64, pre)
    err = float((d["out"].double() - want).abs().max() / want.abs().max())
    checks.append(Check(4, "tail", err < 6e-3, err / 6e-3))
    return checks, dict(v64=v64, y64=y64, want=want)
