"""The three kernels that run on every training iteration -- adam.hip, activations.hip (activations and densification
statistics) and the photometric / depth heads of loss.hip -- against float64 at their edges.

Every bound has one form, elementwise (tests/fused_step_reference.py):

    |hip - f64| <= 2 * |y32 - f64| + floor

`f64` is the float64 reference, `y32` the same expression with every operation rounded to float32 (NumPy) -- what
float32 arithmetic costs for that expression; the factor 2 allows another valid operation order -- and `floor` a
forward-error term derived at each test, never read off a kernel.  Each test prints the worst ratio to its bound
("The per-step kernels against float64", records them).  The references are pinned on torch float64 and
the SSIM oracle in tests/test_fused_step_host.py.

Outputs sit inside larger allocations filled with a sentinel bit pattern (`Guarded`): the guards must survive.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import fused_step_cases as K
import fused_step_reference as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SENTINEL = 0x7FA5C3E1  # a NaN as float32: a kernel that read a guard would also poison its result
GUARD = 256            # elements on either side


class Guarded:
    """A tensor of `shape` inside a sentinel-filled allocation, `offset` elements off the 16-byte alignment."""

    def __init__(self, shape, dtype=torch.float32, offset=0, init=None):
        n = int(np.prod(shape)) if len(shape) else 1
        self.buf = torch.full((GUARD + offset + n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.lo, self.hi = GUARD + offset, GUARD + offset + n
        self.t = self.buf[self.lo:self.hi].view(dtype).reshape(tuple(shape))
        if init is not None:
            self.t.copy_(torch.as_tensor(np.asarray(init)).to(dtype).reshape(self.t.shape))

    def intact(self):
        return bool((self.buf[:self.lo] == SENTINEL).all()) and bool((self.buf[self.hi:] == SENTINEL).all())

    def np(self):
        return self.t.detach().cpu().numpy()


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32)


def native(name, *args):
    from rasterizer.cuda import _call, _stream

    _call(name, *args, _stream(torch.device("cuda", torch.cuda.current_device())))


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------------------------ Adam
def _adam_run(tensors, step, betas, eps):
    """tensors: list of (Guarded p, grad tensor or None, Guarded m, Guarded v, lr).  One FusedAdam.step() from the
    handed-in state at `step - 1`."""
    from gs_fused import FusedAdam

    params = [torch.nn.Parameter(p.t) for p, *_ in tensors]
    for q, (p, g, *_r) in zip(params, tensors):
        assert q.data_ptr() == p.t.data_ptr()
        q.grad = g
    opt = FusedAdam([{"params": [q], "lr": lr} for q, (*_r, lr) in zip(params, tensors)], betas=betas, eps=eps)
    for q, (_p, g, m, v, _lr) in zip(params, tensors):
        if g is not None:
            opt.state[q] = {"step": step - 1, "exp_avg": m.t, "exp_avg_sq": v.t}
    opt.step()
    torch.cuda.synchronize()
    for q, (_p, g, m, v, _lr) in zip(params, tensors):
        if g is not None:  # the handed-in state was used in place
            st = opt.state[q]
            assert st["step"] == step and st["exp_avg"].data_ptr() == m.t.data_ptr()
            assert st["exp_avg_sq"].data_ptr() == v.t.data_ptr()
    return opt


@pytest.mark.parametrize("eps", K.ADAM_EPS)
@pytest.mark.parametrize("betas", K.ADAM_BETAS)
def test_adam_one_step_from_a_handed_in_state(betas, eps):
    """One step from (p, g, m, v, step) over steps 1 .. 10^6, the toolkit's learning rates and the decayed means'
    rate, on tensors that mix the element classes of fused_step_cases.ADAM_CLASSES.

    floor = 1 ulp32(|f64|): the final rounding of each of p, m, v (the other roundings are the yardstick's).
    The tensors with an odd index are views one element off the alignment (scalar path); every p, m, v lies between
    guards; the gradient is read only; all-zero rows come back bit-unchanged."""
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    worst_by_class = np.zeros(len(K.ADAM_CLASSES))
    for si, step in enumerate(K.ADAM_STEPS):
        tensors, host = [], []
        for li, lr in enumerate(K.ADAM_LRS):
            # 7 tensors, one launch; tails of 0-3 elements; two of them (one aligned, one not) need a second workgroup
            n = (4101 if li in (2, 5) else 1500) + 9 * li + (li % 4)
            p, g, m, v, cls = K.adam_elements(n, seed=10 * si + li)
            off = li % 2
            tensors.append((Guarded((n,), offset=off, init=p), cu(g), Guarded((n,), offset=off, init=m),
                            Guarded((n,), offset=off, init=v), lr))
            host.append((p, g, m, v, cls))
        _adam_run(tensors, step, betas, eps)
        for (gp, gg, gm, gv, lr), (p, g, m, v, cls) in zip(tensors, host):
            assert gp.intact() and gm.intact() and gv.intact(), f"step {step} lr {lr}: a guard was written"
            assert np.array_equal(bits(gg), bits(g)), "the gradient was written"
            f64 = R.adam_step(p, g, m, v, step, lr, betas, eps)
            y32 = R.adam_step(p, g, m, v, step, lr, betas, eps, dt=F32)
            hip = (gp.np(), gm.np(), gv.np())
            for nm, h, f, y in zip("pmv", hip, f64, y32):
                worst[nm] = max(worst[nm], R.ratio(h, f, y, R.ulp32(f)))
            for c in range(len(K.ADAM_CLASSES)):
                s = cls == c
                worst_by_class[c] = max(worst_by_class[c], R.ratio(hip[0][s], f64[0][s], y32[0][s], R.ulp32(f64[0][s])))
            z = cls == K.ADAM_CLASSES.index("all_zero")
            assert np.array_equal(bits(hip[0])[z], bits(p)[z]) and not bits(hip[1])[z].any() and not bits(hip[2])[z].any()
    print(f"adam betas {betas} eps {eps}: worst ratio to the bound p {worst['p']:.3f}, m {worst['m']:.3f}, "
          f"v {worst['v']:.3f}; p by class: "
          + ", ".join(f"{nm} {w:.3f}" for nm, w in zip(K.ADAM_CLASSES, worst_by_class)))
    assert max(worst.values()) <= 1.0, worst


def test_adam_update_does_not_depend_on_the_path():
    """The same element values through the float4 body, the tail of up to 3 elements and the scalar path of an unaligned
    view give the same bits (csrc/Makefile: adam.o is built without contraction for exactly this).  Four layouts of the
    same values per size: the tensor as it is (body + tail), padded to a multiple of 4 (all body), rolled by two (other
    elements in the tail), and a view one element off the alignment (all scalar).  13 tensors per optimiser -- two
    launches -- with a zero-size tensor in the middle and a parameter without a gradient."""
    step, betas, eps = 7, (0.9, 0.999), 1e-15
    vals = [K.adam_elements(n, seed=100 + i) for i, n in enumerate(K.PATH_SIZES)]
    lrs = [K.ADAM_LRS[i % len(K.ADAM_LRS)] for i in range(len(vals))]

    def layout(kind):
        ts = []
        for (p, g, m, v, _c), lr in zip(vals, lrs):
            n = p.size
            if kind == "padded":
                pad = (-n) % 4 + 4
                arrs = [np.concatenate([a, a[:1].repeat(pad)]) for a in (p, g, m, v)]
            elif kind == "rolled":
                arrs = [np.roll(a, 2) for a in (p, g, m, v)]
            else:
                arrs = [p, g, m, v]
            off = 1 if kind == "offset" else 0
            gg = Guarded(arrs[1].shape, offset=off, init=arrs[1])
            ts.append((Guarded(arrs[0].shape, offset=off, init=arrs[0]), gg.t, Guarded(arrs[2].shape, offset=off, init=arrs[2]),
                       Guarded(arrs[3].shape, offset=off, init=arrs[3]), lr))
        empty = (Guarded((0,)), torch.empty(0, device="cuda"), Guarded((0,)), Guarded((0,)), 0.01)
        frozen = (Guarded((37,), init=np.arange(37, dtype=F32)), None, Guarded((37,)), Guarded((37,)), 0.01)
        ts.insert(6, empty)
        ts.insert(9, frozen)
        opt = _adam_run(ts, step, betas, eps)
        assert len(opt.param_groups) == 13
        assert all(t[0].intact() and t[2].intact() and t[3].intact() for t in ts)
        assert np.array_equal(frozen[0].np(), np.arange(37, dtype=F32))
        assert (frozen[2].buf == SENTINEL).all() and (frozen[3].buf == SENTINEL).all()  # no state, nothing written
        ts = [t for t in ts if t is not empty and t is not frozen]
        res = []
        for (gp, _g, gm, gv, _lr), (p, *_r) in zip(ts, vals):
            n = p.size
            a = [bits(x.np()) for x in (gp, gm, gv)]
            if kind == "padded":
                a = [x[:n] for x in a]
            elif kind == "rolled":
                a = [np.roll(x, -2) for x in a]
            res.append(a)
        return res

    base = layout("plain")
    for kind in ("padded", "rolled", "offset"):
        other = layout(kind)
        for n, a, b in zip(K.PATH_SIZES, base, other):
            for nm, x, y in zip("pmv", a, b):
                assert np.array_equal(x, y), f"n = {n}: {nm} differs between the plain and the {kind} layout"
    # and the values are right (one size is enough here: the first test holds the values)
    p, g, m, v, _ = vals[-1]
    f64 = R.adam_step(p, g, m, v, step, lrs[-1], betas, eps)
    y32 = R.adam_step(p, g, m, v, step, lrs[-1], betas, eps, dt=F32)
    w = max(R.ratio(h.view(F32), f, y, R.ulp32(f)) for h, f, y in zip(base[-1], f64, y32))
    print(f"adam path independence: 4 layouts x {len(K.PATH_SIZES)} sizes bit-equal; worst ratio at n = {p.size}: {w:.3f}")
    assert w <= 1.0


# ----------------------------------------------------------------------------------------------------- activations
def _activate_native(x, with_dirs=True):
    n = x["log_scales"].shape[0]
    out = dict(scales=Guarded((n, 3)), quats=Guarded((n, 4)), opac=Guarded((n, 1)), dirs=Guarded((n, 3)))
    dev = {k: cu(v) for k, v in x.items()}
    native("gsr_activate_forward", C.c_int(n), ptr(dev["means"]) if with_dirs else None, ptr(dev["log_scales"]),
           ptr(dev["raw_quats"]), ptr(dev["logits"]), ptr(dev["campos"]) if with_dirs else None, ptr(out["scales"].t),
           ptr(out["quats"].t), ptr(out["opac"].t), ptr(out["dirs"].t) if with_dirs else None)
    torch.cuda.synchronize()
    return out, dev


@pytest.mark.parametrize("n", K.ACT_SIZES)
def test_activations_forward_and_backward_at_the_edges(n):
    """Logits to +-104 (sigmoid saturates, exp overflows), log-scales -20 .. 10, quaternion norms 1e-3 .. 1e3
    (axis-aligned, one dominant component, all equal), means 1e-3 and 1e4 from the camera; cotangents parallel,
    anti-parallel and orthogonal to q, zero, random, and None.

    floor = 4 ulp32(|f64|): one expf or sqrtf documented at 1 ulp, the reciprocal and the products correctly rounded
    (half an ulp each), against a yardstick that divides once.  For the quaternion gradient, where v - q (q . v)
    cancels, floor = 8 eps32 (|v| + |q| |q . v|) / |raw| (fused_step_reference.quat_grad_floor)."""
    x = K.activation_inputs(n, seed=n)
    out, dev = _activate_native(x)
    f64 = R.activate_forward(x["means"], x["log_scales"], x["raw_quats"], x["logits"], x["campos"])
    y32 = R.activate_forward(x["means"], x["log_scales"], x["raw_quats"], x["logits"], x["campos"], dt=F32)
    w = {}
    for nm, f, y in zip(("scales", "quats", "opac", "dirs"), f64, y32):
        assert out[nm].intact(), f"forward wrote outside {nm}"
        w[nm] = R.ratio(out[nm].np(), f, y, 4 * R.ulp32(f))
    # without a camera position: the same three outputs, and the view directions are not written
    out2, _ = _activate_native(x, with_dirs=False)
    for nm in ("scales", "quats", "opac"):
        assert np.array_equal(bits(out2[nm].np()), bits(out[nm].np())) and out2[nm].intact()
    assert (out2["dirs"].buf == SENTINEL).all()

    vs, vq, vo = K.activation_cotangents(x["raw_quats"], seed=n + 1)
    f64b = R.activate_vjp(x["log_scales"], x["raw_quats"], x["logits"], vs, vq, vo)
    y32b = R.activate_vjp(x["log_scales"], x["raw_quats"], x["logits"], vs, vq, vo, dt=F32)
    floors = (4 * R.ulp32(f64b[0]), R.quat_grad_floor(x["raw_quats"], vq), 4 * R.ulp32(f64b[2]))

    def backward(cots):
        g = dict(ls=Guarded((n, 3)), rq=Guarded((n, 4)), lo=Guarded((n, 1)))
        d = [None if c is None else cu(c) for c in cots]
        native("gsr_activate_backward", C.c_int(n), ptr(dev["raw_quats"]), ptr(out["scales"].t), ptr(out["quats"].t),
               ptr(out["opac"].t), ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(g["ls"].t), ptr(g["rq"].t), ptr(g["lo"].t))
        torch.cuda.synchronize()
        assert all(t.intact() for t in g.values()), "backward wrote outside its outputs"
        return g

    g = backward((vs, vq, vo))
    for nm, key, f, y, fl in zip(("v_log_scales", "v_raw_quats", "v_logits"), ("ls", "rq", "lo"), f64b, y32b, floors):
        w[nm] = R.ratio(g[key].np(), f, y, fl)
    kinds = np.arange(n) % len(K.COTANGENT_KINDS)
    zero_rows = kinds == K.COTANGENT_KINDS.index("zero")
    assert not g["rq"].np()[zero_rows].any(), "a zero cotangent must give a zero gradient"
    # a None cotangent is exact zeros, and does not disturb the others
    for drop in range(3):
        cots = [vs, vq, vo]
        cots[drop] = None
        gn = backward(cots)
        for k, key in enumerate(("ls", "rq", "lo")):
            if k == drop:
                assert not bits(gn[key].np()).any(), f"{key}: a None cotangent must give +0 everywhere"
            else:
                assert np.array_equal(bits(gn[key].np()), bits(g[key].np()))
    print(f"activations n = {n}: worst ratio to the bound " + ", ".join(f"{k} {v:.3f}" for k, v in w.items()))
    assert max(w.values()) <= 1.0, w


def test_activations_autograd_passes_none_cotangents():
    """Through `activate_gaussians`: a loss that uses one output only hands the kernel None for the other two."""
    from gs_fused import activate_gaussians

    x = K.activation_inputs(257, seed=9)
    ls, rq, lo = (cu(x[k]).requires_grad_(True) for k in ("log_scales", "raw_quats", "logits"))
    s, q, o, dirs = activate_gaussians(None, ls, rq, lo, None)
    assert dirs is None
    vs, vq, vo = K.activation_cotangents(x["raw_quats"], seed=10)
    (q * cu(vq)).sum().backward()
    assert not bits(ls.grad).any() and not bits(lo.grad).any()
    f64 = R.activate_vjp(x["log_scales"], x["raw_quats"], x["logits"], None, vq, None)[1]
    y32 = R.activate_vjp(x["log_scales"], x["raw_quats"], x["logits"], None, vq, None, dt=F32)[1]
    w = R.ratio(rq.grad.cpu().numpy(), f64, y32, R.quat_grad_floor(x["raw_quats"], vq))
    print(f"activations through autograd: v_raw_quats worst ratio {w:.3f}")
    assert w <= 1.0


# ----------------------------------------------------------------------------------------- densification statistics
@pytest.mark.parametrize("device_flag", [False, True], ids=["host_flag", "device_flag"])
@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_densify_stats_both_entry_points(n, device_flag):
    """gsr_densify_stats (`first` on the host) and gsr_densify_stats_dev (`first` read by the kernel, the form the
    backward of render_gaussians uses): radii -1 / 0 / 1 / 300, gradients 1e-12 .. 1e2, a first call over
    accumulators holding NaN and -7, later calls, a call without gradients.

    Counts are exact.  floor = 2 ulp32: the norm is two products, a sum and a square root, the accumulation one more
    sum -- the yardstick performs the same operations, so the floor only has to cover a contracted sum (one rounding
    fewer) and the final rounding.  Invisible rows are bit-unchanged on later calls; guards around the three
    accumulators."""
    from gs_fused import densify_stats_

    size = 1920
    grad, radii = K.densify_inputs(n, seed=n)
    grad2, _ = K.densify_inputs(n, seed=n + 1)
    gn, cnt, mx = Guarded((n,)), Guarded((n,), torch.int32), Guarded((n,))
    gn.t.fill_(float("nan"))
    cnt.t.fill_(-7)
    mx.t.fill_(float("nan"))
    flag = (lambda f: torch.tensor([5 if f else 0], dtype=torch.int32, device="cuda")) if device_flag else (lambda f: f)
    ref64 = ref32 = (np.full(n, np.nan), np.full(n, -7, np.int32), np.full(n, np.nan))
    worst = 0.0
    vis = radii > 0
    for k, (g, first) in enumerate(((grad, True), (grad2, False), (None, False), (grad, False), (None, True))):
        before = [bits(t.np()).copy() for t in (gn, cnt, mx)]
        densify_stats_(None if g is None else cu(g), cu(radii), size, gn.t, cnt.t, mx.t, first=flag(first))
        torch.cuda.synchronize()
        assert gn.intact() and cnt.intact() and mx.intact(), f"call {k}: a guard was written"
        ref64 = R.densify_stats(g, radii, size, *ref64, first)
        ref32 = R.densify_stats(g, radii, size, *ref32, first, dt=F32)
        assert np.array_equal(cnt.np(), ref64[1]), f"call {k}: counts"
        for h, f, y in ((gn.np(), ref64[0], ref32[0]), (mx.np(), ref64[2], ref32[2])):
            worst = max(worst, R.ratio(h, f, y, 2 * R.ulp32(f)))
        if not first:
            for t, b in zip((gn, cnt, mx), before):
                assert np.array_equal(bits(t.np())[~vis], b[~vis]), f"call {k}: an invisible row changed"
            if g is None:
                assert np.array_equal(bits(gn.np()), before[0]), f"call {k}: norms changed without gradients"
    print(f"densify_stats n = {n} {'device' if device_flag else 'host'} flag: worst ratio to the bound {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------- L1 + SSIM
SSIM_CASES = K.ssim_cases()


def _ssim_native(pred, gt, lam, clamp, up):
    H, W, _ = pred.shape
    p, g = cu(pred), cu(gt)
    maps = torch.empty((9, H - 10, W - 10), device="cuda")
    work = torch.empty((128,), dtype=torch.float64, device="cuda")
    loss, terms = Guarded(()), Guarded((2,))
    v_pred = Guarded((H, W, 3))
    native("gsr_l1_ssim_forward", C.c_uint(H), C.c_uint(W), C.c_float(lam), C.c_int(int(clamp)), ptr(p), ptr(g),
           ptr(maps), ptr(work), ptr(loss.t), ptr(terms.t))
    upstream = torch.tensor([up], dtype=torch.float32, device="cuda")
    native("gsr_l1_ssim_backward", C.c_uint(H), C.c_uint(W), C.c_float(lam), C.c_int(int(clamp)), ptr(upstream), ptr(p),
           ptr(g), ptr(maps), ptr(v_pred.t))
    torch.cuda.synchronize()
    assert loss.intact() and terms.intact() and v_pred.intact(), "a guard of the loss head was written"
    assert np.array_equal(bits(p), bits(pred)) and np.array_equal(bits(g), bits(gt))
    return float(loss.np()), terms.np().astype(F64), v_pred.np()


@pytest.fixture(scope="module", params=SSIM_CASES, ids=[c["name"] for c in SSIM_CASES])
def ssim_run(request):
    """One case on the GPU with its references, made once for the tests of this module that take it."""
    case = request.param
    pred, gt, lam, clamp, up = case["pred"], case["gt"], case["lam"], case["clamp"], case["up"]
    x = np.minimum(pred, F32(1)) if clamp else pred
    return dict(case=case, x=x, oracle=O.l1_ssim_loss(x, gt, lam, with_grad=False)[:3],
                f64=R.l1_ssim(pred, gt, lam, clamp, up, with_terms=True), y32=R.l1_ssim(pred, gt, lam, clamp, up, dt=F32),
                hip=_ssim_native(pred, gt, lam, clamp, up))


def test_l1_ssim_head_gradient_on_structured_content(ssim_run):
    """pred == gt, constant pairs (black on black: B1 = C1 = 1e-4), a flat background with one blob, ramps, pred above 1
    with and without the clamp, pred == 1.0, negative pred, saturated images; lambda 0 / 0.2 / 1, upstream != 1; at
    sizes that are one valid position, one tile, one more than a tile (fused_step_cases.SSIM_SIZES).

    The gradient, at every pixel: floor = 32 eps32 sum |terms|, sum |terms| = |L1 term| + every tap's |contribution| to
    the three transposed blurs (float64): 11 + 11 taps plus the pointwise operations, rounded up, each at most one
    rounding of a partial sum no larger than sum |terms|.  Pixels within 1e-6 of x == y without being equal are left
    out (the sign is ill-conditioned there; < 1 % of a case, checked on the host).  Two runs are bit-equal; the clamp
    cuts where pred > 1 and passes at pred == 1.0; guards around v_pred and the scalars (`_ssim_native`)."""
    run, case = ssim_run, ssim_run["case"]
    pred, gt, lam, clamp, up = case["pred"], case["gt"], case["lam"], case["clamp"], case["up"]
    (loss, _terms, v), f_v, terms, y_v = run["hip"], run["f64"][3], run["f64"][4], run["y32"][3]
    keep = ~K.near_tie(pred, gt, clamp) | (run["x"] == gt)
    assert case["equal"] or keep.mean() > 0.99
    w = R.ratio(v[keep], f_v[keep], y_v[keep], 32 * R.EPS32 * terms[keep])
    print(f"l1_ssim {case['name']} {pred.shape[0]}x{pred.shape[1]}: gradient, worst ratio to the bound {w:.3f}; "
          f"{int((~keep).sum())} near-tie values left out")
    if clamp:
        assert not bits(v)[pred > 1].any(), "the clamp cuts the gradient where pred > 1"
    if case["name"].startswith("over_one"):  # pred == 1.0 is not cut (the test is `pred > 1`), with or without the clamp
        assert (pred == 1).any() and (v[pred == 1] != 0).all()
    if case["equal"] and lam == 0:
        assert loss == 0.0 and not v.any(), "pred == gt, lambda 0: the loss and the L1 sign are exactly 0"
    assert np.array_equal(bits(_ssim_native(pred, gt, lam, clamp, up)[2]), bits(v)), "two runs differ in the gradient"
    assert w <= 1.0, w


def test_l1_ssim_head_scalars_on_structured_content(ssim_run):
    """The L1 mean, the SSIM mean and the loss of the same cases against the oracle's doubles, to float32 rounding of
    the result: floor = 1 ulp32 of the value, for each of the three (the final rounding: the kernel forms the loss from
    the two means in double and rounds once).  With pred == gt the oracle's loss is exactly 0, and so must the kernel's
    be: S is exactly 1 there (loss.hip, ssim_point).

    With the window moments in float32 the kernel missed this bound for the SSIM mean (and the loss) in 5 of the 22
    cases -- ratios 1.15 (blob_0.3: 1.5e-5 off, the yardstick 6.5e-6), 1.58, 6.57 (ramp_1), 1.05, 2.18 -- and the
    eight-digit window constants before that put the ramps 5e-6 to 1e-5 off.  The forward kernel now forms the moments
    and S in double (loss.hip)."""
    run, case = ssim_run, ssim_run["case"]
    (loss, (l1, ssim), _v), (o_loss, o_l1, o_ssim), (y_loss, y_l1, y_ssim, _) = run["hip"], run["oracle"], run["y32"]
    fl_l1, fl_ss, fl_loss = float(R.ulp32(o_l1)), float(R.ulp32(o_ssim)), float(R.ulp32(o_loss))
    w = {"l1": R.ratio(l1, o_l1, y_l1, fl_l1), "ssim": R.ratio(ssim, o_ssim, y_ssim, fl_ss),
         "loss": R.ratio(loss, o_loss, y_loss, fl_loss)}
    print(f"l1_ssim {case['name']}: scalars, worst ratio to the bound " + ", ".join(f"{k} {r:.3f}" for k, r in w.items())
          + f"; SSIM mean off by {abs(ssim - o_ssim):.2e} (yardstick {abs(y_ssim - o_ssim):.2e})")
    assert max(w.values()) <= 1.0, w


# ------------------------------------------------------------------------------------------------ L1, depth heads
@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("H,W", K.L1_SHAPES)
def test_l1_head_against_float64(H, W, masked, clamp):
    """n = 3 H W with n % 4 in {0, 1, 2, 3}, n < 4, more than one workgroup; pred == gt, pred == 1.0 and pred > 1
    elements; a non-binary mask.  The loss: floor = 1 ulp32 (its final rounding).  The gradient is a product of at most
    four factors and a sign: floor = 2 ulp32."""
    from gs_fused import l1_loss

    pred, gt, mask = K.l1_case(H, W, seed=3 * H + W)
    weight, up = 0.8, 1.7
    p = cu(pred).requires_grad_(True)
    loss = l1_loss(p, cu(gt), weight, clamp_pred=clamp, mask=cu(mask) if masked else None)
    (loss * up).backward()
    torch.cuda.synchronize()
    m = mask if masked else None
    f_loss, f_g = R.l1_head(pred, gt, weight, clamp, m, up)
    y_loss, y_g = R.l1_head(pred, gt, weight, clamp, m, up, dt=F32)
    w_loss = R.ratio(float(loss.detach()), f_loss, y_loss, R.ulp32(f_loss))
    w_g = R.ratio(p.grad.cpu().numpy(), f_g, y_g, 2 * R.ulp32(f_g))
    print(f"l1 head {H}x{W} masked {masked} clamp {clamp}: worst ratio to the bound loss {w_loss:.3f}, grad {w_g:.3f}")
    g = p.grad.cpu().numpy()
    assert not g[pred == gt].any()
    if clamp:
        assert not g[pred > 1].any()
    assert w_loss <= 1.0 and w_g <= 1.0


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n,covered", [(1, True), (57, True), (2500, True), (57, False)])
def test_depth_head_against_float64(n, covered, masked):
    """alpha == 0 pixels (zero gradients), holes where gt == 0, an image with nothing covered, n = 1, more than one
    workgroup, a non-binary mask.  The loss: floor = 1 ulp32.  The gradients are a sign times a few products and one
    reciprocal: floor = 2 ulp32."""
    from gs_fused import depth_l1_loss

    depth, alpha, gt, mask = K.depth_case(n, seed=n + int(covered), covered=covered)
    up = 0.6
    d, a = cu(depth).requires_grad_(True), cu(alpha).requires_grad_(True)
    loss = depth_l1_loss(d, a, cu(gt), mask=cu(mask) if masked else None)
    (loss * up).backward()
    torch.cuda.synchronize()
    m = mask if masked else None
    f = R.depth_head(depth, alpha, gt, m, up)
    y = R.depth_head(depth, alpha, gt, m, up, dt=F32)
    vd, va = d.grad.cpu().numpy().reshape(-1), a.grad.cpu().numpy().reshape(-1)
    w = (R.ratio(float(loss.detach()), f[0], y[0], R.ulp32(f[0])), R.ratio(vd, f[1], y[1], 2 * R.ulp32(f[1])),
         R.ratio(va, f[2], y[2], 2 * R.ulp32(f[2])))
    print(f"depth head n = {n} covered {covered} masked {masked}: worst ratio to the bound loss {w[0]:.3f}, "
          f"v_depth {w[1]:.3f}, v_alpha {w[2]:.3f}")
    dead = (alpha.reshape(-1) == 0) | (gt.reshape(-1) == 0)
    assert not bits(vd)[dead].any() and not bits(va)[dead].any()
    if not covered:
        assert not vd.any() and not va.any()
    assert max(w) <= 1.0, w
