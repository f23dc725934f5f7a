"""GPU: no model-level entry reads scratch it did not write in the same call, none writes outside the size its query returns, and a
short buffer is refused before anything is launched.

The denoiser's workspace is never cleared and keeps whatever ran before -- another shape, another precision mode (the same
float-sized regions hold fp32, bf16, fp16 or e4m3 data), another routing.  Here every call works in a guarded window of exactly
mdm_workspace_bytes (tests/scratch_hygiene.py) that holds one of three histories -- zeros (Z), a donor run's bytes (D), NaN poison
in every data field with the donor's indices (P) -- and everything the call returns must agree bit for bit between them:
mdm_text_cache_build and mdm_stem_cache_build through the module's own workspace slot, mdm_denoiser_forward with and without the
stem cache, its trace and its MoE counters.  Field names and kinds come from mdm_workspace_layout, the table that carves.

Z twice is the control of every test below.  One path is not repeatable bit for bit, in any mode: the expert_importance counters.
The router's gate kernels (csrc/rowwise.hip, moe_gate*: `atomicAdd(&s_imp[br * E + i], v)`) sum the top-2 probabilities of a
workgroup's rows into LDS with floating-point atomics, whose order changes from run to run; the per-workgroup partials (uimp) are
then summed in a fixed order.  Everything else -- out, every trace slab, expert_usage (integer-valued), the text-side tensors, and
the router's own top_idx / top_val as the last MoE block left them in the workspace -- is bit-equal between two Z runs in all five
modes, as tests/test_module_state_gpu.py relies on.  For expert_importance alone:
  * between fills the addends (top_val) are asserted bit-equal, so two runs can differ by the order of at most `rows` fp32 additions
    of positive terms only: |a - b| <= rows * 2^-24 * max(a, b) per expert (rows = B * T, the most a layer has), asserted under
    every fill in every mode;
  * against the fp64 oracle (oracle/denoiser_ref.py, per sample on its own text tokens) under every fill at the gate
    tests/test_forward_gpu.py holds these counters to, allclose(rtol = 1e-4, atol = 1e-4), in the mode that file gates them in,
    the fp32-grade mode 3 (measured here: at most 5.4e-5 from the oracle, under every fill).  That file has no gate for them in the
    other modes, where the bound above stands: the 16-bit modes route differently from the oracle under free routing, and the
    mixed mode 4 feeds the full-scale router rows that went through fp16 expert GEMMs (measured: 4.4e-4 on a counter of 3.2 at
    D = 1024, over the fp32-grade gate, the same under every fill)."""
import ctypes as C

import pytest
import torch

from conftest import build_module, load_golden, pkg
import scratch_hygiene as SH

pytestmark = pytest.mark.gpu

PRECS = (1, 2, 3, 4, 5)
DONOR_PREC = {1: 4, 2: 3, 3: 2, 4: 1, 5: 3}  # another precision mode, of another 16-bit format where there is one
STEPS = 200  # the stem cache's schedule: one whole 128-step chunk of mdm_stem_cache_build and a partial one

# (case, B, T, N, lengths, text tokens)
S_RAGGED = ("fwd_small_dims", 3, 50, 5, (50, 17, 1), (5, 2, 1))  # 150 / 75 rows: a whole 128-row tile + a partial one | a partial one; T/2 odd
S_FOLD2 = ("fwd_small_dims", 2, 6, 33, (6, 3), None)            # past one fold pass; fewer rows than any tile
S_BIG = ("fwd_big_dims", 2, 20, 5, (20, 7), None)               # the head_dim-256 paths
SHAPES = [S_RAGGED, S_FOLD2, S_BIG]
IDS = ["small-3x50x5", "small-2x6x33", "big-2x20x5"]

_META, _MOD, _DONOR, _ZRES, _INPUTS = {}, {}, {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for d in (_MOD, _DONOR, _ZRES, _INPUTS, _ORACLE):
        d.clear()
    pkg("_lib").lib().mdm_set_gemm_variant(0)


def _module(case, precision):
    if (case, precision) not in _MOD:
        if case not in _META:
            _META[case] = load_golden(case)[1]
        _MOD[case, precision] = build_module(_META[case], precision=precision)[0]
    return _MOD[case, precision]


def _inputs(shape, donor=False):
    """Inputs drawn as in test_forward_shape_sweep_both_modes; the donor's differ in x, timesteps and lengths."""
    key = (shape, donor)
    if key not in _INPUTS:
        case, B, T, N, lengths, tokens = shape
        synth = pkg("synth")
        Dt = _module(case, 3).text_latent_dim
        seed = 300 + B + T + N + (1000 if donor else 0)
        x = synth.uniform_pm1((B, T, 263), "hygiene.x", seed) * (3.0 ** 0.5)
        xf_out = synth.uniform_pm1((B, N, Dt), "hygiene.xf", 300 + B + T + N) * (3.0 ** 0.5)
        gen = torch.Generator().manual_seed(seed)
        ts = torch.randint(0, STEPS, (B,), generator=gen)
        ln = torch.tensor([T + 1 - l for l in lengths] if donor else list(lengths))
        _INPUTS[key] = dict(x=x.cuda(), ts=ts.cuda(), length=ln.cuda(), xf_out=xf_out.cuda(), xf_proj=xf_out.mean(1).cuda(),
                            tokens=list(tokens) if tokens else None)
    return _INPUTS[key]


def _windows(m, shape):
    _, B, T, N, _, _ = shape
    return {"text": (B, 2, N), "stem": (128, 2, 1), "fwd": (B, T, N)}


def _layouts(m, shape):
    pm = m.pack()
    return {k: SH.workspace_layout(pm.model, *btn) for k, btn in _windows(m, shape).items()}


def _counters(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items() if k.endswith(("expert_usage", "expert_importance"))}


def _pipeline(m, shape, inp, prepare, forced=None, stem=True):
    """prepare_text, stem_cache and the forward (without and with the stem cache) of module m, each in a guarded window of exactly the
    queried size that `prepare(kind, window)` has filled; out and trace in guarded allocations; returns every result and the
    windows as the calls left them."""
    case, B, T, N, _, _ = shape
    D = m.latent_dim
    res, guards, left = {}, [], {}
    saved_ws = m._ws

    def window(kind):
        g = SH.guarded(m.workspace_bytes(*_windows(m, shape)[kind]))
        prepare(kind, g.win)
        guards.append((kind, g))
        return g

    try:
        g = window("text")
        m._ws = g.win
        tcache = m.prepare_text(inp["xf_out"], private=True, ntok=inp["tokens"])
        assert m._ws is g.win, "prepare_text must have worked in the window"
        left["text"] = g.win
        for i, t in enumerate(tcache["keep"][:3] + tcache["keep"][5:]):
            res[f"text_cache.{i}"] = t
        sc = None
        if stem:
            g = window("stem")
            m._ws, m._time_table = g.win, None
            sc = m.stem_cache(STEPS, inp["xf_proj"])
            assert m._ws is g.win, "stem_cache must have worked in the window"
            left["stem"] = g.win
            res["stem.table"], res["stem.gx"] = sc["keep"]
    finally:
        m._ws = saved_ws
    for name, cache in (("", None), ("stem.", sc)):
        if name and cache is None:
            continue
        g = window("fwd")
        go, out = SH.guarded_like((B, T, 263), fill=7.0)
        gt, tr = SH.guarded_like((2 * m.num_layers, 4, B * T, D), fill=7.0)
        guards += [(name + "out", go), (name + "trace", gt)]
        m.reset_all_moe_counters()
        before = _counters(m)
        y, t = m(inp["x"], inp["ts"], inp["length"], xf_proj=inp["xf_proj"], xf_out=inp["xf_out"], workspace=g.win, trace=tr,
                 out=out, forced_routing=forced, text_cache=tcache, stem_cache=cache)
        assert y.data_ptr() == out.data_ptr() and t.data_ptr() == tr.data_ptr()
        res[name + "out"], res[name + "trace"] = y, t
        for k, v in _counters(m).items():
            res[f"{name}counter.{k}"] = v - before[k]
        left[name + "fwd"] = g.win
        for fname, off, size, _ in SH.workspace_layout(m.pack().model, B, T, N):
            if fname in ("top_idx", "top_val"):  # of the last MoE block, the full-scale layer: 2 branches x B T rows x 2
                res[f"{name}ws.{fname}"] = g.win[off:off + size].view(torch.int32).clone()
    torch.cuda.synchronize()
    for kind, g in guards:
        assert g.guards_untouched(), f"{kind}: a write outside the window of {g.nbytes} bytes"
    return res, left


def _donor(shape, precision):
    """The bytes a donor run leaves in the three windows: the same width and (B, T, N), other x / timesteps / lengths, free routing,
    precision DONOR_PREC[precision], from zeroed windows."""
    q = DONOR_PREC[precision]
    key = (shape, q)
    if key not in _DONOR:
        _, left = _pipeline(_module(shape[0], q), shape, _inputs(shape, donor=True), lambda kind, win: win.zero_())
        _DONOR[key] = {k: left[k].clone() for k in ("text", "stem", "fwd")}
    return _DONOR[key]


def _run(shape, precision, fill, forced=None, stem=True):
    """The pipeline's results under `fill`.  Under P the run must also have been in the poison's presence: in every window some data
    field is still mostly poison afterwards (nothing cleared the window behind the test's back); those fields are printed."""
    m = _module(shape[0], precision)
    lay = _layouts(m, shape)
    donor = _donor(shape, precision) if fill != "Z" else None
    res, left = _pipeline(m, shape, _inputs(shape), lambda kind, win: SH.fill_window(win, fill, lay[kind], donor and donor[kind]),
                          forced=forced, stem=stem)
    if fill == "P":
        for kind, win in left.items():
            layout = lay[kind.split(".")[-1]]
            data = {n for n, _, _, k in layout if k == 0}
            kept = {n: f for n, f in SH.poison_fraction(win, layout).items() if n in data and f > 0.5}  # (chance 0xFF bytes: 0.4 %)
            print(f"{shape[:4]} precision {precision} {kind}: mostly poison after the call: " + ", ".join(f"{n} {f:.0%}" for n, f in kept.items()))
            assert kept, f"{kind}: no data field kept its poison: the fill was not there during the call"
    return res


def _run_or_skip(shape, precision, fill, **kw):
    L = pkg("_lib")
    try:
        return _run(shape, precision, fill, **kw)
    except L.MdmError as e:
        if precision != L.PREC_FP8:
            raise
        pytest.skip(f"precision {precision} refused at {shape[0]}: {e}")


def _z(shape, precision):
    if (shape, precision) not in _ZRES:
        _ZRES[shape, precision] = {k: v.clone() for k, v in _run_or_skip(shape, precision, "Z").items()}
    return _ZRES[shape, precision]


_ORACLE = {}


def _oracle_importance(shape):
    """{state_dict key of an expert_importance buffer: its increment over one forward} from the oracle, free routing; every sample
    run alone on its own text tokens (the oracle takes no token counts; samples do not interact), increments summed."""
    if shape not in _ORACLE:
        import os, sys
        from conftest import ROOT, golden_state
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import denoiser_ref as R
        case, B, T, N, _, _ = shape
        _module(case, 3)
        sd, eph, proj, mcfg = golden_state(_META[case])
        inp = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in _inputs(shape).items()}
        total = {}
        for b in range(B):
            n = inp["tokens"][b] if inp["tokens"] else N
            trace = {}
            with torch.no_grad():
                R.denoiser_forward(sd, mcfg, inp["x"][b:b + 1], inp["ts"][b:b + 1], inp["length"][b:b + 1], inp["xf_proj"][b:b + 1],
                                   inp["xf_out"][b:b + 1, :n], eph, proj, None, trace)
            for scale in ("low", "high"):
                for br in range(2):
                    pre = f"decoder_blocks_{scale}.0.module.ffn.branches.{br}"
                    v = trace[pre + ".importance"].float()
                    total[pre + ".moe.expert_importance"] = total.get(pre + ".moe.expert_importance", 0) + v
        _ORACLE[shape] = total
    return _ORACLE[shape]


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16) if t.is_floating_point() else t


def _compare(label, want, got, fill, rows):
    """Every result of `got` (a run under `fill`) equals `want` (the Z run).  out / trace / expert_usage by torch.equal -- a NaN fails
    it; the text-side tensors and the router's top_idx / top_val bit for bit; expert_importance within the reordering bound of
    a sum of at most `rows` equal addends (the module docstring)."""
    assert want.keys() == got.keys()
    bad = []
    for k in want:
        a, b = want[k], got[k]
        if k.endswith("expert_importance"):
            same = bool(((a - b).abs() <= rows * 2.0 ** -24 * torch.maximum(a.abs(), b.abs())).all())
        elif "out" in k or "trace" in k or "counter" in k:
            same = torch.equal(a, b)
        else:
            same = torch.equal(_bits(a), _bits(b))
        if not same:
            nan = int(torch.isnan(b.float()).sum())
            diff = int((_bits(a) != _bits(b)).sum())
            bad.append(f"{k}: {diff} of {a.numel()} elements differ, {nan} NaN")
    assert not bad, f"{label}: fill {fill} against Z: " + "; ".join(bad)


@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_results_do_not_depend_on_the_workspace_contents(shape, precision):
    """prepare_text, stem_cache, forward(trace) and forward(stem_cache, trace) under Z, Z again (the control: every path is
    repeatable bit for bit), D and P: out, trace, the MoE counters' increments and the text-side tensors are equal; no guard of a
    workspace window, of out or of trace is touched."""
    want = _z(shape, precision)
    assert torch.isfinite(want["out"]).all() and torch.isfinite(want["stem.out"]).all()
    assert not bool((want["out"] == 7.0).all())
    for fill in ("Z", "D", "P"):
        got = _run_or_skip(shape, precision, fill)
        _compare(f"{shape[:4]} precision {precision}", want, got, fill, shape[1] * shape[2])
        if precision == 3:
            for k, ref in _oracle_importance(shape).items():
                for pre in ("counter.", "stem.counter."):
                    v = got[pre + k].cpu()
                    print(f"{shape[:4]} precision {precision} fill {fill} {pre}{k}: max |d| vs oracle {float((v - ref).abs().max()):.2e}")
                    assert torch.allclose(v, ref, rtol=1e-4, atol=1e-4), (fill, pre + k, v, ref)


# knob of mdm_set_gemm_variant -> the modes in which tests/test_attention_selective_gpu.py / test_blocks_gpu.py (and the knobs' own
# files) run it against the default path; 23 exists at head_dim 256 only
KNOB_MODES = {22: (1, 2), 24: (1, 2), 34: (1, 2, 4), 35: (1, 2), 50: (1, 2), 51: (1, 2), 52: (3, 4), 56: (3, 4), 60: (3, 4), 61: (3, 4),
              62: (3, 4), 171: (1, 2), 172: (1, 2), 174: (1, 2)}
KNOB_CASES = [(S_RAGGED, k, p) for k, ps in sorted(KNOB_MODES.items()) for p in ps] + [(S_BIG, 23, 1), (S_BIG, 23, 2)]


@pytest.mark.parametrize("shape,knob,precision", KNOB_CASES, ids=[f"knob{k}-p{p}" for _, k, p in KNOB_CASES])
def test_reference_path_knobs_do_not_depend_on_the_workspace_contents(shape, knob, precision):
    """The chains behind the knobs use sub-buffers the fused paths leave alone (scr, kvt, phi, qkv, f1): Z against P, text side
    included (the knob is set for the whole pipeline)."""
    lib = pkg("_lib").lib()
    _donor(shape, precision)  # (made on the default path)
    assert lib.mdm_set_gemm_variant(knob) == 0
    try:
        want = _run(shape, precision, "Z")
        got = _run(shape, precision, "P")
    finally:
        lib.mdm_set_gemm_variant(0)
    assert torch.isfinite(want["out"]).all()
    print(f"knob {knob} precision {precision} {shape[:4]}: exercised")
    _compare(f"knob {knob} precision {precision}", want, got, "P", shape[1] * shape[2])


def _forced(shape, name):
    """forced_routing [2 L][2 branches][rows of the layer][2], L = 1 (coarse layer: B T / 2 rows, then padding).
    pair01:   every row of both branches -> experts (0, 1): six of a branch's eight groups stay empty;
    one_last: the first row of each branch -> (E - 1, 0), every other row -> (0, 1): one row on the last expert."""
    _, B, T, _, _, _ = shape
    E = 8
    fr = torch.zeros((2, 4 * B * T), dtype=torch.int32)
    for li, M in enumerate((B * T // 2, B * T)):
        idx = torch.zeros((2, M, 2), dtype=torch.int32)
        idx[:, :, 1] = 1
        if name == "one_last":
            idx[:, 0, 0], idx[:, 0, 1] = E - 1, 0
        fr[li, :idx.numel()] = idx.reshape(-1)
    return fr.cuda()


@pytest.mark.parametrize("routing", ["pair01", "one_last"])
@pytest.mark.parametrize("precision", [1, 3, 5])
def test_empty_and_skewed_experts(precision, routing):
    """Expert groups that receive no row, or one: what the slab kernels leave unwritten there must not reach a result."""
    shape = S_RAGGED
    fr = _forced(shape, routing)
    want = _run_or_skip(shape, precision, "Z", forced=fr, stem=False)
    assert torch.isfinite(want["out"]).all()
    free = _z(shape, precision)
    assert not torch.equal(want["out"], free["out"]), "the forced routing must change the forward"
    for fill in ("Z", "D", "P"):
        _compare(f"routing {routing} precision {precision}", want, _run(shape, precision, fill, forced=fr, stem=False), fill,
                 shape[1] * shape[2])


def _direct(m, shape, inp, tcache, ws, ws_bytes, out):
    L = pkg("_lib")
    _, B, T, _, _, _ = shape
    ln = inp["length"].to(torch.int32)
    return L.lib().mdm_denoiser_forward(C.byref(m.pack().model), C.byref(tcache["tc"]), inp["x"].data_ptr(), inp["ts"].data_ptr(),
                                        ln.data_ptr(), inp["xf_proj"].data_ptr(), B, T, out.data_ptr(), ws.data_ptr(), ws_bytes,
                                        None, None, None, m.precision, L.stream_ptr())


@pytest.mark.parametrize("precision", [1, 3])
def test_a_short_workspace_is_refused_before_any_launch(precision):
    """ws_bytes = need - 1 on mdm_denoiser_forward, mdm_text_cache_build (need(B, 2, N) - 1) and mdm_block_forward: MDM_ERR_ARG, out
    keeps its sentinel, the window its fill and the guards theirs; the same call with ws_bytes = need succeeds (so the size is what
    was refused)."""
    L = pkg("_lib")
    lib = L.lib()
    shape = S_RAGGED
    _, B, T, N, _, _ = shape
    m = _module(shape[0], precision)
    pm = m.pack()
    inp = _inputs(shape)
    tcache = m.prepare_text(inp["xf_out"], private=True, ntok=inp["tokens"])
    FILL = 0xC3

    def refused_then_taken(call, need, out_shape):
        g = SH.guarded(need)
        go, out = SH.guarded_like(out_shape, fill=7.0)
        g.win.fill_(FILL)
        assert call(g.win, need - 1, out) == SH.ERR_ARG
        torch.cuda.synchronize()
        assert bool((g.win == FILL).all()), "a refused call wrote into the workspace"
        assert bool((out == 7.0).all()), "a refused call wrote its output"
        assert g.guards_untouched() and go.guards_untouched()
        g.win.zero_()  # (the refusal's fill is no valid index: the call that runs starts from zeros)
        assert call(g.win, need, out) == 0
        torch.cuda.synchronize()
        assert g.guards_untouched() and go.guards_untouched()
        return out

    y = refused_then_taken(lambda ws, n, out: _direct(m, shape, inp, tcache, ws, n, out), m.workspace_bytes(B, T, N), (B, T, 263))
    assert torch.isfinite(y).all() and not bool((y == 7.0).all())

    # mdm_text_cache_build: its outputs are the cache's tensors; sd_k [2 L, B, N, D] stands for them
    D, H, L2 = m.latent_dim, m.num_heads, 2 * m.num_layers
    at = torch.empty((L2, B, H, D // H, D // H), device="cuda")
    sv = torch.empty((L2, B, N, D), device="cuda")

    def text_build(ws, n, sk):
        tc = L.TextCache()
        tc.lin_at, tc.sd_k, tc.sd_v, tc.B, tc.N = at.data_ptr(), sk.data_ptr(), sv.data_ptr(), B, N
        return lib.mdm_text_cache_build(C.byref(pm.model), inp["xf_out"].data_ptr(), C.byref(tc), ws.data_ptr(), n, precision,
                                        L.stream_ptr())

    sk = refused_then_taken(text_build, m.workspace_bytes(B, 2, N), (L2, B, N, D))
    assert torch.equal(sk, tcache["keep"][1])

    # mdm_block_forward, the whole coarse layer on S = T / 2 frames
    S = T // 2
    synth = pkg("synth")
    h = (synth.uniform_pm1((B, S, D), "hygiene.h", 1) * 1.5).cuda()
    sc = synth.uniform_pm1((4, B, 2 * D), "hygiene.sc", 1).cuda() * 0.5
    ln = torch.tensor([S, 8, 1], dtype=torch.int32).cuda()

    def block(ws, n, out):
        return lib.mdm_block_forward(C.byref(pm.model), 0, L.BLOCK_LAYER, C.byref(tcache["tc"]), h.data_ptr(), sc.data_ptr(),
                                     ln.data_ptr(), B, S, out.data_ptr(), ws.data_ptr(), n, None, precision, L.stream_ptr())

    y = refused_then_taken(block, m.workspace_bytes(B, S, N), (B, S, D))
    assert torch.isfinite(y).all()


# the three (B, T, N, lengths, tokens) of the table above on one width
def _history_shapes(case):
    return [(case,) + s[1:] for s in SHAPES]


@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("case", ["fwd_small_dims", "fwd_big_dims"])
def test_shape_history(case, precision):
    """One module, one window sized for the largest of the three shapes, poisoned once at the start (P by the layout of the first
    shape to run); then the three shapes in two different orders, each forward working in the leading bytes of the window as the
    run before it left them.  Every result equals the Z result of its shape.  Before each run the int fields of that run's own
    layout take a donor's in-range values (poison and leftovers of another layout never stand where an index is expected: whether
    a stale index is read is the business of Z against D above); every data field keeps its history."""
    shapes = _history_shapes(case)
    m = _module(case, precision)
    want = [_z(s, precision) for s in shapes]
    need = [m.workspace_bytes(s[1], s[2], s[3]) for s in shapes]
    lays = [SH.workspace_layout(m.pack().model, s[1], s[2], s[3]) for s in shapes]
    donors = [_donor(s, precision)["fwd"] for s in shapes]
    g = SH.guarded(max(need))
    g.win.fill_(SH.POISON_BYTE)
    for i in (0, 1, 2, 1, 0, 2, 0):
        s, inp = shapes[i], _inputs(shapes[i])
        _, B, T, N, _, _ = s
        SH.copy_int_fields(g.win, lays[i], donors[i])
        tcache = m.prepare_text(inp["xf_out"], private=True, ntok=inp["tokens"])
        go, out = SH.guarded_like((B, T, 263), fill=7.0)
        behind = g.win[need[i]:].clone()
        y = m(inp["x"], inp["ts"], inp["length"], xf_proj=inp["xf_proj"], xf_out=inp["xf_out"], workspace=g.win[:need[i]], out=out,
              text_cache=tcache)
        torch.cuda.synchronize()
        assert g.guards_untouched() and go.guards_untouched()
        assert torch.equal(g.win[need[i]:], behind), f"shape {s[1:4]} wrote behind its {need[i]} bytes"
        assert torch.equal(y, want[i]["out"]), (f"{case} precision {precision}: shape {s[1:4]} after the runs before it",
                                               int(torch.isnan(y).sum()), int((y != want[i]["out"]).sum()))
