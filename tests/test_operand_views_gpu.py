"""GPU: the GEMM and fused-MLP kernels on strided operand views (tests/operand_views.py).

Every operand of MdmGemmDesc / MdmMlpDesc is a pointer and a leading dimension, and the model relies on it (16-bit rows with
A.ld = nblk * Te, C16 windows of kfold / vfold, (scale | shift) rows with ldc = 2 D); the dense tests pass ld = width everywhere.
Here every input is a window of a NaN-poisoned allocation and every output a window of a sentinel-filled one:

  aligned windows  every kernel family, forced by its documented knob, on the views and on contiguous copies of the same values:
                   the two results agree in every bit (same kernel, tile and path), the result is within the gate the dense test
                   of that kernel uses against fp64 of the identically rounded operands, nothing outside an output window changed;
  odd ld           the element-wise fallbacks of gemm2.hip / gemm3.hip and the launches knobs 6 / 68 / 70 must hand on: fp64 gate,
                   canary, finite (the element-wise paths add the residuals in another order: no bit equality);
  refusals         mdm_fused_mlp with an odd ldc or an unaligned b1: MDM_ERR_UNSUPPORTED and nothing written;
  packers          the ld_src / ldw arguments of the five packers, through the C ABI.

tests/test_operand_views_host.py proves that these assertions see each stride confusion on these windows."""
import ctypes as C

import pytest
import torch

import operand_views as V
from conftest import pkg

pytestmark = pytest.mark.gpu


def _mods():
    return pkg("_lib"), pkg("ops")


class _Knob:
    def __init__(self, knob):
        self.knob = knob

    def __enter__(self):
        pkg("_lib").lib().mdm_set_gemm_variant(self.knob)

    def __exit__(self, *exc):
        pkg("_lib").lib().mdm_set_gemm_variant(0)


_ACT = {"none": 0, "gelu": 1, "silu": 2, "feat": 3}


def _packed(c, t, knob):
    """(PackedWeight, weight stream or None) of a case; the stream only where the knob's kernel has one."""
    L, ops = _mods()
    w = t.w.cuda() if len(c.sizes) > 1 else t.w[0].cuda()
    pw = ops.PackedWeight(w, fmt="f16") if c.a_fmt == "f16" else ops.PackedWeight(w)
    ws = None
    if knob in (63, 68):  # a launch the streamed kernel cannot take still carries a stream (of the first 256 columns): never read
        ws = ops.gemm_stream1_pack(t.w[0, :c.N // 256 * 256].cuda(), V.H16[c.a_fmt])
    elif knob in (69, 70):
        ws = ops.gemm_stream3x_pack(t.w[:, :c.N // 512 * 512].cuda())
    assert knob not in (63, 68, 69, 70) or ws is not None
    return pw, ws


def _launch(c, o, pw, ws):
    """One mdm_gemm of the operand set `o` (operand_views.on_device)."""
    L, ops = _mods()
    d = ops.gemm_desc(c.precision)
    if c.a_fmt in V.H16:
        d.A.p, d.A.ld, d.A.kind = o.A.view.data_ptr(), o.A.ld, L.OP_BF16_ROW
        d.precision, d.h16 = 1, (L.H16_F16 if c.a_fmt == "f16" else L.H16_BF16)
    elif c.a_fmt == "f32":
        d.A = ops.f32_operand(o.A.view, o.A.ld)
    else:  # pre-split rows: ld in 4-byte units
        d.A = ops.f32_operand(o.A.view, o.A.ld // 2)
        d.A.kind = L.OP_X2_ROW
    d.A.gather = L.ptr(o.gather)
    d.W = pw.operand()
    d.w_stream = L.ptr(ws)
    d.M, d.N, d.K = c.M, c.N, c.K
    if len(c.sizes) > 1:
        d.goff, d.ngroups, d.W.bs1, d.bias_bs = o.goff.data_ptr(), len(c.sizes), c.N * pw.Kp, c.N
        if ws is not None:
            d.w_stream_gs = L.lib().mdm_gemm_stream3x_group_elems(C.c_int32(c.N // 512 * 512), C.c_int32(c.K))
    d.bias, d.act, d.alpha, d.out_scale = o.bias.data_ptr(), _ACT[c.act], c.alpha, c.out_scale
    d.colscale, d.rowscale = L.ptr(o.colscale), L.ptr(o.rowscale)
    if o.R1 is not None:
        d.R1, d.ldr1, d.r1_scale, d.r1_mod = o.R1.view.data_ptr(), o.R1.ld, c.r1_scale, c.r1_mod
    if o.R2 is not None:
        d.R2, d.ldr2 = o.R2.view.data_ptr(), o.R2.ld
    if o.C is not None:
        d.C, d.ldc = o.C.view.data_ptr(), o.C.ld
    if o.C16 is not None:
        d.C16, d.ldc = o.C16.view.data_ptr(), o.C16.ld
    if o.Cx2 is not None:
        d.Cx2, d.ldc = o.Cx2.view.data_ptr(), o.Cx2.ld // 2
    for w in (o.A, o.R1, o.R2, o.C, o.C16, o.Cx2):  # misaligned base pointers are out of scope: never handed to a GPU here
        assert w is None or w.view.data_ptr() % 16 == 0
    ops.run_gemm(d)


@pytest.mark.parametrize("name", sorted(V.ALIGNED))
def test_aligned_windows_are_bit_equal_to_the_dense_run(name):
    c, knob, kernel = V.ALIGNED[name]
    t = V.build_gemm(c)
    pw, ws = _packed(c, t, knob)
    view, dense = V.on_device(t, "cuda"), V.on_device(t, "cuda", dense=True)
    with _Knob(knob):
        _launch(c, view, pw, ws)
        _launch(c, dense, pw, ws)
    torch.cuda.synchronize()
    V.gemm_checks(f"{name} [{kernel}]", view, dense)


@pytest.mark.parametrize("name", sorted(V.ODD))
def test_odd_leading_dimensions_and_unaligned_vectors(name):
    c, knob, kernel = V.ODD[name]
    t = V.build_gemm(c)
    pw, ws = _packed(c, t, knob)
    view = V.on_device(t, "cuda")
    assert (view.bias.data_ptr() % 16 == 4) == (c.layout == "vec_off")
    with _Knob(knob):
        _launch(c, view, pw, ws)
    torch.cuda.synchronize()
    V.gemm_checks(f"{name} [{kernel}]", view)


def _rand(g, *shape, scale=1.0):
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


@pytest.mark.parametrize("act", ["none", "headnorm"])
def test_gemm3_plane_outputs_in_a_wider_buffer(act):
    """csrc/gemm3.hip: the C16 / C16_lo plane pair with ldc > N, MDM_ACT_NONE (alpha, residual) and MDM_ACT_HEADNORM (head_dim 128,
    the first two of the three slices L2-normalised); gates of test_plane_outputs_and_head_softmax_epilogue /
    test_headnorm_epilogue_writes_normalised_hi_lo_planes."""
    import torch.nn.functional as F
    L, ops = _mods()
    M, N, K = 200, 384, 64
    g = torch.Generator().manual_seed(11)
    x, w, b = _rand(g, M, K), _rand(g, N, K, scale=K ** -0.5), _rand(g, N, scale=0.1)
    hw, hb = 1 + 0.2 * _rand(g, 128), 0.1 * _rand(g, 128)
    A = V.in_aligned(M, K).put(x)
    R1 = V.in_aligned(M, N, extra=64).put(_rand(g, M, N))
    pw = ops.PackedWeight(w.cuda())
    bd, hwd, hbd = b.cuda(), hw.cuda(), hb.cuda()
    base = x.double() @ w.double().T + b.double()
    if act == "none":
        ref = 0.25 * base + 0.5 * R1.view.double()
    else:
        ref = F.layer_norm((0.1 * base).reshape(M, 3, 128), (128,), hw.double(), hb.double(), 1e-5)
        ref[:, :2] = F.normalize(ref[:, :2], dim=-1)
        ref = ref.reshape(M, N)
    runs = []
    for dense in (False, True):
        a, r1 = (A.dense("cuda"), R1.dense("cuda")) if dense else (A.to("cuda"), R1.to("cuda"))
        ld, col0 = (N, 0) if dense else (N + 32, 32)
        hi, lo = V.out_window(M, N, torch.bfloat16, ld, col0).to("cuda"), V.out_window(M, N, torch.bfloat16, ld, col0).to("cuda")
        d = ops.gemm_desc(3)
        d.A = ops.f32_operand(a.view, a.ld)
        d.W = pw.operand()
        d.M, d.N, d.K = M, N, K
        d.bias = bd.data_ptr()
        if act == "none":
            d.act, d.alpha = L.ACT_NONE, 0.25
            d.R1, d.ldr1, d.r1_scale = r1.view.data_ptr(), r1.ld, 0.5
        else:
            d.act, d.alpha = L.ACT_HEADNORM, 0.1
            d.hn_w, d.hn_b, d.hn_l2_tiles = hwd.data_ptr(), hbd.data_ptr(), 2
        d.C16, d.C16_lo, d.ldc = hi.view.data_ptr(), lo.view.data_ptr(), ld
        ops.run_gemm(d)
        runs.append((hi, lo))
    torch.cuda.synchronize()
    (hi, lo), (dhi, dlo) = runs
    outs = [V.Out(name="hi", got=hi.view, dense=dhi.view, ref=ref if act == "headnorm" else None, tol=5e-3),
            V.Out(name="lo", got=lo.view, dense=dlo.view, ref=None, tol=None),
            V.Out(name="hi+lo", got=hi.view.double() + lo.view.double(), dense=None, ref=ref, tol=3e-5)]
    V.check_case(f"gemm3 planes {act} [gemm3.hip]", outs, [hi, lo])


@pytest.mark.parametrize("grouped", [False, True])
def test_fp8_gemm_on_a_wider_byte_buffer(grouped):
    """csrc/gemm8.hip through ops.gemm_fp8: the e4m3 rows inside a wider 0x7f (= NaN) buffer with ld % 16 == 0, fp32 and e4m3
    outputs as windows; 200 x 256 x 256 dense, and grouped [130, 0, 70] with a row gather.  Gates of tests/test_fp8_gpu.py."""
    L, ops = _mods()
    M, N, K, S = 200, 256, 256, (90 if grouped else 200)
    g = torch.Generator().manual_seed(12)
    G = 3 if grouped else 1
    src, w, b = _rand(g, S, K, scale=2.0), _rand(g, G, N, K, scale=K ** -0.5), _rand(g, G, N, scale=0.1)
    rs = (_rand(g, M).abs() + 0.1).cuda()
    a8, asc = ops.quantize_rows_fp8(src.cuda())
    pw = ops.PackedWeight((w if grouped else w[0]).cuda(), fmt="f8")
    bd = (b if grouped else b[0]).cuda()
    goff = torch.tensor([0, 130, 130, 200], dtype=torch.int32).cuda() if grouped else None
    gather = torch.randint(0, S, (M,), generator=g, dtype=torch.int32).cuda() if grouped else None
    A = V.Win(S, K, ld=K + 64, col0=32, dtype=torch.uint8, fill=V.FP8_NAN, device="cuda").put(a8)
    assert A.ld % 16 == 0 and A.view.data_ptr() % 16 == 0
    runs = []
    for dense in (False, True):
        a = A.dense() if dense else A
        ld, col0 = (N, 0) if dense else (N + 32, 32)
        out = V.out_window(M, N, torch.float32, ld, col0).to("cuda")
        out8 = V.out_window(M, N, torch.uint8, ld, col0).to("cuda")
        ops.gemm_fp8(a.view, asc, pw, bd, act=L.ACT_GELU, rowscale=rs, gather=gather, goff=goff, rows=M, out=out.view, out8=out8.view,
                     c8_scale=8.0)
        runs.append((out, out8))
    torch.cuda.synchronize()
    (out, out8), (dout, dout8) = runs
    deq = lambda q8, sc: q8.view(torch.float8_e4m3fn)[:, :K].double() * sc.double()[:, None]  # noqa: E731
    xq = deq(a8, asc)
    xq = xq[gather.long()] if grouped else xq
    wq = deq(pw.hi, pw.lo).reshape(G, N, K)
    ref = torch.empty(M, N, dtype=torch.float64, device="cuda")
    bounds = [0, 130, 130, 200] if grouped else [0, M]
    for e in range(G):
        r = slice(bounds[e], bounds[e + 1])
        ref[r] = torch.nn.functional.gelu(xq[r] @ wq[e].T + bd.reshape(G, N)[e].double())
    ref = ref * rs.double()[:, None]
    V.check_case(f"fp8 {'grouped' if grouped else 'dense'} [gemm8.hip]",
                 [V.Out(name="C", got=out.view, dense=dout.view, ref=ref, tol=2e-5), V.Out(name="C8", got=out8.view, dense=dout8.view, ref=None, tol=None)],
                 [out, out8])
    # the e4m3 copy is the rounded fp32 result: only rounding-boundary ties may differ (test_grouped_gathered_fp8_mlp_chain)
    want8 = (out.view * 8.0).to(torch.float8_e4m3fn).float()
    assert float((out8.view.view(torch.float8_e4m3fn).float() != want8).float().mean()) < 2e-3


_MLP_TOL = {torch.bfloat16: 3e-3, torch.float16: 6e-4}  # tests/test_mlp_gpu.py


def _mlp_setup(dtype, grouped):
    ops = pkg("ops")
    Din, F, Dout = 128, 256, 512
    sizes = [65, 0, 12] if grouped else [77]
    G, M, S = len(sizes), sum(sizes), (40 if grouped else 77)
    g = torch.Generator().manual_seed(13)
    p = dict(Din=Din, F=F, Dout=Dout, sizes=sizes, G=G, M=M, S=S, grouped=grouped, dtype=dtype)
    x16 = _rand(g, S, Din).to(dtype)
    p["w1"], p["b1"] = _rand(g, G, F, Din, scale=Din ** -0.5), _rand(g, G, F, scale=0.1)
    p["w2"], p["b2"] = _rand(g, G, Dout, F, scale=F ** -0.5), _rand(g, G, Dout, scale=0.1)
    p["X"] = V.in_aligned(S, Din, dtype).put(x16)
    p["R1"] = V.in_aligned(M, Dout, extra=64).put(_rand(g, M, Dout))
    p["R2"] = V.in_aligned(M, Dout, extra=96).put(_rand(g, M, Dout))
    p["rs"] = _rand(g, M).abs() + 0.1 if grouped else None
    p["gather"] = torch.randint(0, S, (M,), generator=g, dtype=torch.int32) if grouped else None
    p["goff"] = torch.tensor([0] + list(torch.tensor(sizes).cumsum(0)), dtype=torch.int32) if grouped else None
    rd = lambda t: t.to(dtype).double()  # noqa: E731
    xs = x16.double()[p["gather"].long()] if grouped else x16.double()
    ref = torch.empty(M, Dout, dtype=torch.float64)
    o = 0
    for e, n in enumerate(sizes):
        h = torch.nn.functional.gelu(xs[o:o + n] @ rd(p["w1"][e]).T + p["b1"][e].double())
        ref[o:o + n] = rd(h.float()) @ rd(p["w2"][e]).T + p["b2"][e].double()
        o += n
    if grouped:
        ref = ref * p["rs"].double()[:, None]
    p["ref"] = ref + 0.5 * p["R1"].view.double() + p["R2"].view.double()
    fmt = "f16" if dtype == torch.float16 else "bf16"
    sq = (lambda t: t.cuda()) if grouped else (lambda t: t[0].cuda())
    p["pw1"], p["pw2"] = ops.PackedWeight(sq(p["w1"]), fmt=fmt), ops.PackedWeight(sq(p["w2"]), fmt=fmt)
    p["ws"] = ops.mlp_stream_pack(sq(p["w1"]), sq(p["w2"]), dtype)
    p["b1d"], p["b2d"] = sq(p["b1"]), sq(p["b2"])
    return p


def _mlp_run(p, dense, *, ldc=None, b1=None, only16=False, made=None):
    """One mdm_fused_mlp on the windows (or their contiguous copies); returns the output windows (C or None, C16), which are also
    appended to `made` before the call (a refused call raises)."""
    ops = pkg("ops")
    dt, M, Dout = p["dtype"], p["M"], p["Dout"]
    X, R1, R2 = ((w.dense("cuda") if dense else w.to("cuda")) for w in (p["X"], p["R1"], p["R2"]))
    ld, col0 = (Dout, 0) if dense else (Dout + 32, 32)
    if ldc is not None:
        ld, col0 = ldc, 0
    Cw = None if only16 else V.out_window(M, Dout, torch.float32, ld, col0).to("cuda")
    C16 = V.out_window(M, Dout, dt, ld, col0).to("cuda")
    dev = lambda t: None if t is None else t.cuda()  # noqa: E731
    for w in (X, R1, R2, Cw, C16):
        assert w is None or w.view.data_ptr() % 16 == 0
    outs = (Cw, C16)
    if made is not None:
        made.extend(w for w in outs if w is not None)
    ops.fused_mlp(X.view, p["pw1"], p["b1d"] if b1 is None else b1, p["pw2"], p["b2d"], gather=dev(p["gather"]), goff=dev(p["goff"]),
                  rowscale=dev(p["rs"]), r1=R1.view, r1_scale=0.5, r2=R2.view, rows=M, out=None if Cw is None else Cw.view, out16=C16.view,
                  wstream=p["ws"], only16=only16)
    return outs


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("knob,kernel", [(34, "mlp.hip"), (0, "mlp_stream.hip")])
def test_fused_mlp_on_windows(knob, kernel, dtype, grouped):
    """csrc/mlp.hip (knob 34) and csrc/mlp_stream.hip: X rows with ldx = Din + 64, R1 / R2 / C with three different leading
    dimensions, dense M = 77 and grouped [65, 0, 12] with a row gather; fp32 + 16-bit outputs and the 16-bit-only epilogue; the
    canary includes the rows past M."""
    p = _mlp_setup(dtype, grouped)
    with _Knob(knob):
        C32, C16 = _mlp_run(p, False)
        D32, D16 = _mlp_run(p, True)
        _, only = _mlp_run(p, False, only16=True)
        _, donly = _mlp_run(p, True, only16=True)
    torch.cuda.synchronize()
    tol = _MLP_TOL[dtype]
    tol16 = 1e-2 if (knob == 34 and dtype == torch.bfloat16) else 4 * tol
    label = f"fused MLP {'grouped' if grouped else 'dense'} {str(dtype)[6:]} [{kernel}]"
    V.check_case(label, [V.Out(name="C", got=C32.view, dense=D32.view, ref=p["ref"], tol=tol),
                         V.Out(name="C16", got=C16.view, dense=D16.view, ref=p["ref"], tol=tol16)], [C32, C16])
    V.check_case(label + " only16", [V.Out(name="C16", got=only.view, dense=donly.view, ref=p["ref"], tol=tol16)], [only],
                 derived=[("only16 vs the 16-bit copy", only.view, C16.view)])


@pytest.mark.parametrize("knob,kernel", [(34, "mlp.hip"), (0, "mlp_stream.hip")])
@pytest.mark.parametrize("what", ["odd_ldc", "b1_off"])
def test_fused_mlp_refuses_what_its_vector_paths_cannot_take(what, knob, kernel):
    """ldc = Dout + 1, or b1 one element into a longer vector: both kernels store / load 16 bytes there, so mdm_fused_mlp returns
    MDM_ERR_UNSUPPORTED before any launch and every output buffer keeps every bit."""
    L = pkg("_lib")
    p = _mlp_setup(torch.bfloat16, False)
    if what == "odd_ldc":
        kw = dict(ldc=p["Dout"] + 1)
    else:
        kw = dict(b1=V.offset_vector(p["b1"][0].cuda()))
        assert kw["b1"].data_ptr() % 16 == 4
    made = []
    with _Knob(knob):
        for only16 in (False, True):
            with pytest.raises(L.MdmError, match="MDM_ERR_UNSUPPORTED"):
                _mlp_run(p, False, only16=only16, made=made, **kw)
    torch.cuda.synchronize()
    assert len(made) == 3
    for w in made:  # not one bit of any output allocation changed, inside the window or outside
        assert V.outside_untouched(w.buffer, (0, 0, 0), w.fill)


# ---- packers, through the C ABI -------------------------------------------------------------------------------------------------
def _filled(n, dtype):
    return torch.full((n,), 0x55, dtype=torch.uint8, device="cuda").view(dtype)


@pytest.mark.parametrize("K", [40, 300])
def test_row_packers_read_through_ld_src(K):
    """mdm_pack_bf16 (with the lo plane), mdm_pack_f16, mdm_pack_fp8 with ld_src = K + 5 on a NaN-poisoned source: bit-equal to the
    pack of the contiguous copy, zero padding and fp8 scales included."""
    L = pkg("_lib")
    lib, rows = L.lib(), 37
    g = torch.Generator().manual_seed(14)
    src = V.Win(rows, K, ld=K + 5, col0=0, device="cuda").put(_rand(g, rows, K, scale=3.0).cuda())
    con = src.view.contiguous()
    k32, k128 = (K + 31) // 32 * 32, (K + 127) // 128 * 128
    res = []
    for t, ld in ((src.view, K + 5), (con, K)):
        hi, lo, h16 = _filled(rows * k32 * 2, torch.bfloat16), _filled(rows * k32 * 2, torch.bfloat16), _filled(rows * k32 * 2, torch.float16)
        q8, sc = _filled(rows * k128, torch.uint8), _filled(rows * 4, torch.float32)
        L.check(lib.mdm_pack_bf16(t.data_ptr(), ld, rows, K, hi.data_ptr(), lo.data_ptr(), k32, L.stream_ptr()), "mdm_pack_bf16")
        L.check(lib.mdm_pack_f16(t.data_ptr(), ld, rows, K, h16.data_ptr(), k32, L.stream_ptr()), "mdm_pack_f16")
        L.check(lib.mdm_pack_fp8(t.data_ptr(), ld, rows, K, q8.data_ptr(), k128, sc.data_ptr(), L.stream_ptr()), "mdm_pack_fp8")
        res.append((hi, lo, h16, q8, sc))
    torch.cuda.synchronize()
    for name, a, b in zip(("bf16 hi", "bf16 lo", "f16", "fp8", "fp8 scales"), *res):
        assert torch.equal(V.bits(a), V.bits(b)), name
    hi, lo, h16, q8, sc = res[0]
    want_hi = con.to(torch.bfloat16)
    assert torch.equal(V.bits(hi.view(rows, k32)[:, :K]), V.bits(want_hi)) and not V.bits(hi.view(rows, k32)[:, K:]).any()
    assert torch.equal(V.bits(lo.view(rows, k32)[:, :K]), V.bits((con - want_hi.float()).to(torch.bfloat16))) and not V.bits(lo.view(rows, k32)[:, K:]).any()
    assert torch.equal(V.bits(h16.view(rows, k32)[:, :K]), V.bits(con.to(torch.float16))) and not V.bits(h16.view(rows, k32)[:, K:]).any()
    assert torch.allclose(sc, con.abs().amax(1) / 448.0, rtol=1e-6) and not q8.view(rows, k128)[:, K:].any()
    assert torch.isfinite(q8.view(torch.float8_e4m3fn).float()).all()  # (tests/test_fp8_gpu.py holds the bytes against torch's rounding)


def test_stream_packers_read_through_ldw():
    """mdm_gemm_stream1_pack (both 16-bit formats) and mdm_gemm_stream3x_pack with ldw = K + 32 on a NaN-poisoned source: bit-equal
    to the stream of the contiguous copy, skew and tail padding included."""
    L = pkg("_lib")
    lib = L.lib()
    g = torch.Generator().manual_seed(15)
    N, K, G = 512, 512, 2
    src = V.Win(G * N, K, ld=K + 32, col0=0, device="cuda").put(_rand(g, G * N, K).cuda())
    con = src.view.contiguous()
    n1, n3 = lib.mdm_gemm_stream1_elems(N, K), lib.mdm_gemm_stream3x_elems(G, N, K)
    assert n1 > 0 and n3 > 0
    res = []
    for t, ld in ((src.view, K + 32), (con, K)):
        outs = []
        for h16, dt in ((L.H16_BF16, torch.bfloat16), (L.H16_F16, torch.float16)):
            o = _filled(2 * n1, dt)
            L.check(lib.mdm_gemm_stream1_pack(t.data_ptr(), ld, N, K, h16, o.data_ptr(), L.stream_ptr()), "mdm_gemm_stream1_pack")
            outs.append(o)
        o = _filled(2 * n3, torch.bfloat16)
        L.check(lib.mdm_gemm_stream3x_pack(t.data_ptr(), ld, G, N, K, o.data_ptr(), L.stream_ptr()), "mdm_gemm_stream3x_pack")
        outs.append(o)
        res.append(outs)
    torch.cuda.synchronize()
    for name, a, b in zip(("stream1 bf16", "stream1 f16", "stream3x"), *res):
        assert a.numel() in (n1, n3) and torch.isfinite(a.float()).all(), name
        assert torch.equal(V.bits(a), V.bits(b)), name
