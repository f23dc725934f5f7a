"""GPU: the step outside the decoder layers against the oracle, stage by stage, on the fixtures of tests/frame_probe.py: the plain
stem (mdm_stem_embeddings), the stem cache (mdm_stem_cache_build, gated_mix_gather), joint_embed + sequence_embedding + down with
the halved lengths, up + skip, the output head and the text cache (mdm_text_cache_build), in precisions 3, 4, 2 and 1.

Every stage is teacher-forced: it is checked given the device's own upstream tensors (its (scale | shift) rows, its trace of the
block in front), so 16-bit noise does not accumulate across stages and no stage reads a tensor behind a routing decision -- no
routing has to be injected.  Every gate is MARGIN x frame_probe.MEASURED[stage][width][precision], the error of the oracle under
a rounding hook measured on the CPU; tests/test_frame_probe_host.py shows from the oracle alone that every mutant of
frame_probe is at least POWER such tolerances away.  The project's whole-tensor bounds (1e-3 fp32-grade, TOL of
tests/test_blocks_gpu.py) are asserted beside them."""
import ctypes as C

import pytest
import torch

from conftest import pkg, rel_inf
from test_blocks_gpu import TOL

import frame_probe as FP

pytestmark = pytest.mark.gpu

_MOD, _REF = {}, {}
WIDTH_PRECISION = [(w, p) for w in FP.FRAME_WIDTHS for p in FP.PRECISIONS[w]]


def _module(width, precision):
    """The model on the fixture's weights (kept: 14 in all, the largest about 1 GB)."""
    if (width, precision) not in _MOD:
        fs = FP.frame_state(width)
        cfg = fs["meta"]["cfg"]
        m = pkg("transformer").MotionTransformer(
            cfg["input_feats"], num_frames=cfg["num_frames"], latent_dim=cfg["latent_dim_arg"], ff_size=cfg["ff_size_arg"],
            num_layers=cfg["num_layers"], num_heads=cfg["num_heads"], text_latent_dim=cfg["text_latent_dim_arg"],
            moe_num_experts=cfg["moe_num_experts"], model_size=cfg["model_size"], precision=precision)
        m.load_state_dict(fs["sd"], strict=True)
        m.set_ephemerals(fs["eph"])
        m.set_projections(fs["proj"])
        _MOD[width, precision] = m.cuda().eval()
    return _MOD[width, precision]


def _memo(key, fn):
    if key not in _REF:
        with torch.no_grad():
            _REF[key] = fn()
    return _REF[key]


def _device_stem(m, ts, xp):
    """(emb (B, D), sc (8L, B, 2D)) of mdm_stem_embeddings."""
    L = pkg("_lib")
    pm = m.pack()
    B, D = len(ts), m.latent_dim
    ts_d, xp_d = ts.to(torch.int64).cuda(), xp.cuda().contiguous()
    emb = torch.empty((B, D), device="cuda")
    sc = torch.empty((8 * m.num_layers, B, 2 * D), device="cuda")
    ws = m._workspace(B, 2, 1)
    L.check(L.lib().mdm_stem_embeddings(C.byref(pm.model), C.c_void_p(ts_d.data_ptr()), C.c_void_p(xp_d.data_ptr()), C.c_int32(B),
                                        C.c_void_p(emb.data_ptr()), C.c_void_p(sc.data_ptr()), C.c_void_p(ws.data_ptr()),
                                        C.c_int64(ws.numel()), C.c_int32(m.precision), C.c_void_p(L.stream_ptr())))
    return emb.cpu(), sc.cpu()


@pytest.mark.parametrize("width,precision", [(w, p) for w in ("tiny",) + FP.FRAME_WIDTHS for p in FP.PRECISIONS[w]])
def test_plain_stem_rows_match_the_oracle(width, precision):
    """mdm_stem_embeddings at B in {1, 3, 33, 130}, timesteps 0, 1, 998, 999 and a repeated one: emb and each of the 8L (scale |
    shift) slots against R.fused_embedding and the per-slot Linears in f64, rel_inf per (slot, sample) row."""
    m = _module(width, precision)
    fs64 = FP.as64(FP.frame_state(width))
    gate = FP.tol("stem", width, precision)
    bad = []
    for B in FP.STEM_BATCHES:
        ts, xp = FP.stem_inputs(width, B)
        ref = _memo(("stem", width, B), lambda: FP.stem(fs64, ts, xp))
        got = _device_stem(m, ts, xp)
        rows_e, rows_s = FP.rows_rel(got[0], ref[0]), FP.rows_rel(got[1], ref[1])
        whole = max(rel_inf(got[0], ref[0]), rel_inf(got[1], ref[1]))
        print(f"stem {width} B={B} precision {precision}: worst row of emb {rows_e:.2e}, of the (scale | shift) slots {rows_s:.2e} "
              f"(gate {gate:.1e}), whole {whole:.2e} (gate {TOL[precision]:.0e})")
        if not (rows_e < gate and rows_s < gate and whole < TOL[precision]):
            bad.append((B, rows_e, rows_s, whole))
    assert not bad, bad


@pytest.mark.parametrize("width", FP.FRAME_WIDTHS)
def test_stem_cache_table_and_text_half_match_the_oracle_in_every_mode(width):
    """mdm_stem_cache_build: steps = 300 (three chunks of the 128-row builder, the last of 44 rows; 130 at the big width) and
    B = 130 rows of gx (two chunks): every table row against the oracle's proj_time(...) chain and every gx row against
    proj_text(...), at the fp32-grade tolerance in every mode, and bit-equal across the modes.  (The module keeps the table per
    (steps, packed weights): whichever test of this file asks first has the builder fill it.)"""
    fs64 = FP.as64(FP.frame_state(width))
    steps = FP.STEM_CACHE_STEPS[width]
    _, xp = FP.stem_inputs(width, FP.STEM_CACHE_BATCH)
    ref = _memo(("cache", width), lambda: FP.stem_cache(fs64, steps, xp))
    seen, bad = {}, []
    for p in FP.PRECISIONS[width]:
        m = _module(width, p)
        table, gx = (t.cpu() for t in m.stem_cache(steps, xp.cuda())["keep"])
        et, eg = FP.rows_rel(table, ref[0]), FP.rows_rel(gx, ref[1])
        gate = FP.tol("stem_cache", width, p)
        print(f"stem cache {width} precision {p}: worst table row {et:.2e}, worst gx row {eg:.2e} (gate {gate:.1e})")
        if not (et < gate and eg < gate and rel_inf(table, ref[0]) < 1e-3 and rel_inf(gx, ref[1]) < 1e-3):
            bad.append((p, et, eg))
        seen[p] = (table, gx)
    assert not bad, bad
    first = seen[FP.PRECISIONS[width][0]]
    for p, (table, gx) in seen.items():
        assert torch.equal(table, first[0]) and torch.equal(gx, first[1]), f"the stem cache of precision {p} differs"


def _slot(tr, li, slot, B, S, D):
    M = B * S
    return tr[li].reshape(-1)[slot * M * D:(slot + 1) * M * D].reshape(B, S, D).cpu()


def _forward(m, inp, width, **kw):
    fs = FP.frame_state(width)
    xf = pkg("synth").uniform_pm1((inp["B"], 6, fs["Dt"]), "frame.gpu.xf", inp["T"]) * (3.0 ** 0.5)
    return m(inp["x"].cuda(), inp["ts"].cuda(), inp["length"].cuda(), xf_proj=inp["xp"].cuda(), xf_out=xf.cuda(), trace=True, **kw)


def _judge(bad, label, fs, out, ref, base, length, stage, width, precision):
    whole, branch, blockwise = FP.branch_metric(fs, out, ref, base, length)
    gate = FP.tol(stage, width, precision)
    print(f"{label}: whole {whole:.2e} (gate {TOL[precision]:.0e})  branch {branch:.2e}  worst (sample, head block) {blockwise:.2e} "
          f"(gate {gate:.1e})")
    if not (whole < TOL[precision] and branch < gate and blockwise < gate):
        bad.append((label, whole, branch, blockwise))


@pytest.mark.parametrize("width,precision", WIDTH_PRECISION)
def test_embedding_down_up_and_head_match_the_oracle(width, precision):
    """One traced forward per case of frame_probe.CASES, three stages read from it:
    embed_down -- slot 0 of layer 0 against the oracle's dual block on the oracle's h_low under the oracle's coarse mask;
    up_skip    -- the device's last coarse block through the oracle's conv_transpose1d, plus the oracle's h_embed, through the
                  oracle's dual block of the first full-scale layer, against slot 0 of layer L (on fwd_tools_shape this pins the
                  (L - 1) and L offsets of the trace and of the (scale | shift) rows);
    head       -- the oracle's `out` Linear in f64 on the device's last block against the output, per sample over all T frames.
    The two dual blocks get the device's own (scale | shift) rows (mdm_stem_embeddings on the same inputs)."""
    m = _module(width, precision)
    fs, fs64 = FP.frame_state(width), FP.as64(FP.frame_state(width))
    L, D = fs["L"], fs["D"]
    bad = []
    for case in FP.cases_of(width):
        inp = FP.frame_inputs(width, case)
        B, T = inp["B"], inp["T"]
        _, sc = _device_stem(m, inp["ts"], inp["xp"])
        y, tr = _forward(m, inp, width)
        label = f"{width} B={B} T={T} lengths {case[2]} precision {precision}"
        with torch.no_grad():
            _judge(bad, "embed_down " + label, fs, _slot(tr, 0, 0, B, T // 2, D), FP.read_low(fs, inp, inp["h_low"], sc=sc),
                   inp["base_lo"], inp["len_low"], "embed_down", width, precision)
            hc = FP.up_skip(fs, _slot(tr, L - 1, 3, B, T // 2, D), inp["h"])
            _judge(bad, "up_skip " + label, fs, _slot(tr, L, 0, B, T, D), FP.read_high(fs, inp, hc, sc=sc),
                   FP.dual_base(fs, hc, "high"), inp["length"], "up_skip", width, precision)
            ref = FP.head(fs64, _slot(tr, 2 * L - 1, 3, B, T, D).double())
        per, whole, gate = FP.per_sample_rel(y.cpu(), ref), rel_inf(y.cpu(), ref), FP.tol("head", width, precision)
        print(f"head {label}: worst sample {per:.2e} (gate {gate:.1e}), whole {whole:.2e} (gate {TOL[precision]:.0e})")
        if not (per < gate and whole < TOL[precision]):
            bad.append(("head " + label, per, whole))
    assert not bad, bad


@pytest.mark.parametrize("width,precision", WIDTH_PRECISION)
def test_forward_with_and_without_the_stem_cache(width, precision):
    """The same step through the plain stem and through gated_mix_gather on a stem cache, per-sample timesteps on the chunk edges
    of the table (rows 0, 127, 128, 255, 256 and steps - 1; at the big width's 130 steps 0, 1, 127, 128 and 129): both against
    the oracle's block-0 trace with nothing given, in the block0 tolerance, and against each other in the stem_pair tolerance
    (how far two correct stems put that tensor apart: the dual block's own rounding is the same in both).  What the two claim
    about a gather one row off:
    tests/test_frame_probe_host.py::test_a_gather_one_row_off_is_seen_between_the_two_forwards_in_every_mode."""
    m = _module(width, precision)
    fs = FP.frame_state(width)
    inp = FP.frame_inputs(width, FP.PAIR_CASE, ts=FP.pair_timesteps(width))
    B, T = inp["B"], inp["T"]
    cache = m.stem_cache(FP.STEM_CACHE_STEPS[width], inp["xp"].cuda())
    bad, slot0 = [], {}
    for label, kw in (("plain stem", {}), ("stem cache", {"stem_cache": cache})):
        _, tr = _forward(m, inp, width, **kw)
        slot0[label] = _slot(tr, 0, 0, B, T // 2, fs["D"])
        _judge(bad, f"block 0, {label}, {width} precision {precision}", fs, slot0[label], inp["lo"], inp["base_lo"],
               inp["len_low"], "block0", width, precision)
    _judge(bad, f"block 0, stem cache against plain stem, {width} precision {precision}", fs, slot0["stem cache"], slot0["plain stem"],
           inp["base_lo"], inp["len_low"], "stem_pair", width, precision)
    assert not bad, bad


@pytest.mark.parametrize("width", FP.FRAME_WIDTHS)
def test_text_cache_slabs_match_the_oracle_for_every_layer_in_every_mode(width):
    """mdm_text_cache_build through prepare_text: lin_at against R.linear_cross_text_state and sd_k / sd_v against the key / value
    Linears of the softmax cross-attention, for every one of the 2L layers, N in {1, 6, 33, 85, 128}, B = 3 with token counts
    (N, N - 1, 1) and junk of 9 x the token scale past each count: the reference of a sample is the oracle on exactly its own
    tokens.  fp32-grade tolerance in every mode, the slabs bit-equal across the modes (sd_k / sd_v up to each count: the rows
    past it are unspecified)."""
    fs64 = FP.as64(FP.frame_state(width))
    bad = []
    for N in FP.TEXT_N:
        xf, ntok = FP.text_inputs(width, N)
        ref = _memo(("text", width, N), lambda: FP.text_state(fs64, xf, ntok))
        seen = {}
        for p in FP.PRECISIONS[width]:
            m = _module(width, p)
            at, sk, sv = (t.cpu() for t in m.prepare_text(xf.cuda(), private=True, ntok=ntok)["keep"][0:3])
            got = (at.transpose(-1, -2), sk, sv)  # include/mdm_hip.h: lin_at holds A^T of fast_attention.py:252
            err, gate = FP.text_metric(got, ref, ntok), FP.tol("text_cache", width, p)
            print(f"text cache {width} N={N} tokens {ntok} precision {p}: worst (layer, sample) {err:.2e} (gate {gate:.1e})")
            own = torch.arange(N)[None, :] < torch.tensor(ntok)[:, None]  # (B, N): a sample's own tokens
            whole = max(rel_inf(got[0], ref[0]), *(rel_inf(got[s][:, own], ref[s][:, own]) for s in (1, 2)))
            if not (err < gate and whole < 1e-3):
                bad.append((N, p, err, whole))
            seen[p] = got
        first = seen[FP.PRECISIONS[width][0]]
        for p, got in seen.items():
            assert torch.equal(got[0], first[0]), f"lin_at of precision {p} differs at N = {N}"
            for b, n in enumerate(ntok):
                assert torch.equal(got[1][:, b, :n], first[1][:, b, :n]) and torch.equal(got[2][:, b, :n], first[2][:, b, :n]), (p, N, b)
    assert not bad, bad
