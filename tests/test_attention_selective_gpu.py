"""GPU: every attention core against the oracle on the probe fixtures of tests/attention_probe.py -- inputs on which a wrong
key mask, head or frame pairing, feature map, clamp or token count moves the result -- with metrics over the valid frames that
the residual does not swamp: the whole tensor (the project's tolerances), the branch alone, and the worst (sample, block of
head_dim columns) of the branch.  The branch tolerances are 4 x the error of the oracle under a rounding hook, measured on the
CPU (attention_probe.MEASURED); tests/test_attention_probe_host.py shows from the oracle alone that every mutant is at least
4 x the tolerance away at the precisions listed here.  Every path of perf_core_path, lin_xattn_path and sd_path (csrc/model.hip)
is reached through the variant knobs of include/mdm_hip.h."""
import ctypes as C

import pytest
import torch

from conftest import pkg
from test_blocks_gpu import TOL, _run_block

import attention_probe as AP

pytestmark = pytest.mark.gpu

# include/mdm_hip.h MDM_VAR_*
VAR_SD_UNFOLDED, VAR_GENERIC_DH256, VAR_SD_FOLD_ANY, VAR_TAIL_SPLIT = 22, 23, 24, 35
VAR_QKV_SPLIT, VAR_XQ_SPLIT, VAR_X3_ATTN_CHAIN, VAR_X3_XATTN_CHAIN = 50, 51, 52, 56

# the precisions each fixture variant runs in (the `clamp` variant passes 0.1 e^15, which fp16 does not hold: DESIGN.md section 2)
PRECISIONS = {"mid": (3, 4, 2, 1), "clamp": (3, 4, 1)}
BIG_PRECISIONS = (3, 4, 2, 1)


def branch_gate(kind, variant, precision, width="small"):
    return AP.branch_tol(kind, variant, precision, width)


def self_paths(precision, S, width="small"):
    """(knob, label) of the Performer core paths this precision has at this shape (csrc/model.hip perf_core_path).  The labels
    restate that chooser (the library does not report the path it took): whoever changes perf_core_path, lin_xattn_path or
    sd_path changes them here.  The knob is what selects; a stale label would misname a case, not skip a path."""
    if width == "big":
        return [(0, "CORE256"), (VAR_GENERIC_DH256, "CHAIN")] if precision in (1, 2) else [(0, "CHAIN")]
    if precision in (1, 2):
        return ([(0, "CORE16_QKV")] if S <= 208 else []) + [(VAR_QKV_SPLIT, "CORE16")]
    return [(0, "CORE3"), (VAR_X3_ATTN_CHAIN, "CHAIN")]


_MOD = {}


def _module(width, variant, precision):
    """The model on the fixture's weights (the two most recent are kept: the tests walk the cases of one module in a row)."""
    key = (width, variant, precision)
    if key not in _MOD:
        while len(_MOD) >= 2:
            _MOD.pop(next(iter(_MOD)))
        sd, eph, proj, H, D, Dt, meta = AP.selective_state(width, variant)
        cfg = meta["cfg"]
        m = pkg("transformer").MotionTransformer(
            cfg["input_feats"], num_frames=cfg["num_frames"], latent_dim=cfg["latent_dim_arg"], ff_size=cfg["ff_size_arg"],
            num_layers=cfg["num_layers"], num_heads=cfg["num_heads"], text_latent_dim=cfg["text_latent_dim_arg"],
            moe_num_experts=cfg["moe_num_experts"], model_size=cfg["model_size"], precision=precision)
        m.load_state_dict(sd, strict=True)
        m.set_ephemerals(eph)
        m.set_projections(proj)
        _MOD[key] = m.cuda().eval()
    return _MOD[key]


_REF = {}


def _oracle(kind, width, variant, case):
    key = (kind, width, variant, case)
    if key not in _REF:
        fx = AP.selective_state(width, variant)
        inp = AP.selective_inputs(width, *case)
        _REF[key] = (AP.reference(kind, fx, inp), AP.base_of(kind, fx, inp))
    return _REF[key]


def _run_performer(m, which, inp, N=1):
    L = pkg("_lib")
    pm = m.pack()
    B, S = inp["B"], inp["S"]
    ws = m._workspace(B, S, N)
    hd, ld = inp["h"].cuda().contiguous(), inp["length"].to(torch.int32).cuda()
    sc = inp["sc"][which].cuda().contiguous()
    out = torch.empty_like(hd)
    L.check(L.lib().mdm_performer_attn_forward(C.byref(pm.model), C.c_int32(0), C.c_int32(which), C.c_void_p(hd.data_ptr()),
                                               C.c_void_p(sc.data_ptr()), C.c_void_p(ld.data_ptr()), C.c_int32(B), C.c_int32(S),
                                               C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_int64(ws.numel()),
                                               C.c_int32(m.precision), C.c_void_p(L.stream_ptr())))
    return out.cpu()


def _with_knob(knob, fn):
    lib = pkg("_lib").lib()
    lib.mdm_set_gemm_variant(knob)
    try:
        return fn()
    finally:
        lib.mdm_set_gemm_variant(0)


def _judge(bad, label, out, kind, width, variant, case, precision, past=True):
    ref, base = _oracle(kind, width, variant, case)
    inp = AP.selective_inputs(width, *case)
    H = AP.selective_state(width, variant)[3]
    whole, branch, blockwise = AP.metrics(out, ref, base, inp["length"], H)
    gate = branch_gate(kind, variant, precision, width)
    print(f"{label}: whole {whole:.2e} (gate {TOL[precision]:.0e})  branch {branch:.2e}  worst (sample, head block) {blockwise:.2e} "
          f"(gate {gate:.1e})")
    if not (whole < TOL[precision] and branch < gate and blockwise < gate):
        bad.append((label, whole, branch, blockwise))
    if past:
        try:
            AP.check_past_length(out, ref, inp["length"], TOL[precision])
        except AssertionError as e:
            bad.append((label, str(e)))


def _self_params():
    return [(v, p) for v in ("mid", "clamp") for p in PRECISIONS[v]]


@pytest.mark.parametrize("variant,precision", _self_params())
def test_performer_entry_on_selective_inputs(variant, precision):
    """mdm_performer_attn_forward, both attention slots, every core path of the precision, S in {224, 196, 98, 37, 17, 5}, per launch
    a full, an S - 1, tile-edge, a one-frame and an empty sample."""
    m = _module("small", variant, precision)
    bad = []
    for case in (AP.SELF_CASES if variant == "mid" else AP.CLAMP_CASES):
        inp = AP.selective_inputs("small", *case)
        for knob, path in self_paths(precision, case[0]):
            for which in (0, 1):
                out = _with_knob(knob, lambda: _run_performer(m, which, inp))
                _judge(bad, f"performer {which} {variant} S={case[0]} lengths {case[1]} precision {precision} path {path} (knob {knob})",
                       out, f"performer{which}", "small", variant, case, precision)
    assert not bad, bad


@pytest.mark.parametrize("variant,precision", _self_params())
def test_dual_block_on_selective_inputs(variant, precision):
    """MDM_BLOCK_DUAL through mdm_block_forward on the same cases: every core path, and in the 16-bit modes both forms of the
    projection / stylization tail (MDM_VAR_TAIL_SPLIT)."""
    m = _module("small", variant, precision)
    L = pkg("_lib")
    bad = []
    for case in (AP.SELF_CASES if variant == "mid" else AP.CLAMP_CASES):
        inp = AP.selective_inputs("small", *case)
        paths = self_paths(precision, case[0]) + ([(VAR_TAIL_SPLIT, "default core, tail split")] if precision in (1, 2) else [])
        for knob, path in paths:
            out = _with_knob(knob, lambda: _run_block(m, L.BLOCK_DUAL, inp["h"], inp["sc"], inp["length"], inp["xf"]))
            _judge(bad, f"dual {variant} S={case[0]} lengths {case[1]} precision {precision} path {path} (knob {knob})", out, "dual",
                   "small", variant, case, precision)
    assert not bad, bad


@pytest.mark.parametrize("precision", BIG_PRECISIONS)
def test_big_width_performer_entry_on_selective_inputs(precision):
    """head_dim 256: the two-launch core of csrc/perf_attn2.hip and the GEMM-composed chain (MDM_VAR_GENERIC_DH256).

    The fp16 chain is the case this test was first to see: a model packed for fp16 holds P as one fp16 plane, and the chain's
    feature GEMM, which works on fp32 rows, read that plane as bf16 (error of the size of the whole branch, invisible with the
    seeded P, whose logits of +-0.1 leave the core an average of V).  The chain now re-splits the plane (csrc/model.hip)."""
    m = _module("big", "mid", precision)
    bad = []
    for case in AP.BIG_CASES:
        inp = AP.selective_inputs("big", *case)
        for knob, path in self_paths(precision, case[0], "big"):
            for which in (0, 1):
                out = _with_knob(knob, lambda: _run_performer(m, which, inp))
                _judge(bad, f"big performer {which} S={case[0]} lengths {case[1]} precision {precision} path {path} (knob {knob})", out,
                       f"performer{which}", "big", "mid", case, precision)
    assert not bad, bad


@pytest.mark.parametrize("precision", PRECISIONS["mid"])
def test_text_cross_attentions_on_selective_inputs(precision):
    """MDM_BLOCK_CROSS (query projection inside the launch and split; xattn3 and its chain) and MDM_BLOCK_SDCROSS (folded at any N,
    unfolded core / chain, the default policy; xattn3 and its chain) with per-sample token counts N, N - 1 and 1, junk-like rows
    past each count, N in {1, 6, 28, 64, 65, 85, 96, 128}; the reference of a sample is the oracle on exactly its own tokens.
    Rows past a sample's length are not looked at here (past=False): these blocks work row by row -- a frame's result depends
    on its own row and the text only, the length does not enter them -- so such a row is one more query row like the valid
    ones, and the launch-wide empty and one-frame samples belong to the self-attention tests above."""
    m = _module("small", "mid", precision)
    L = pkg("_lib")
    bad = []
    if precision in (1, 2):
        paths = {"cross": [(0, "CORE_Q"), (VAR_XQ_SPLIT, "CORE")],
                 "sd": [(0, "default"), (VAR_SD_FOLD_ANY, "FOLD"), (VAR_SD_UNFOLDED, "CORE / CHAIN")]}
    else:
        paths = {k: [(0, "CORE3 (xattn3)"), (VAR_X3_XATTN_CHAIN, "CHAIN")] for k in ("cross", "sd")}
    for case in AP.TEXT_CASES:
        inp = AP.selective_inputs("small", *case)
        for kind, block in (("cross", L.BLOCK_CROSS), ("sd", L.BLOCK_SDCROSS)):
            for knob, path in paths[kind]:
                out = _with_knob(knob, lambda: _run_block(m, block, inp["h"], inp["sc"], inp["length"], inp["xf"], ntok=inp["ntok"]))
                _judge(bad, f"{kind} S={case[0]} N={case[2]} tokens {case[3]} precision {precision} path {path} (knob {knob})", out, kind,
                       "small", "mid", case, precision, past=False)
    assert not bad, bad
