"""The fused policy kernel (csrc/policy_mlp.hip) held to a float64 model of its arithmetic (tests/helpers.py policy_model, the
contract of include/swarm_policy.h), at every kind of shape the C ABI accepts, both precisions, fp32 and bf16 rows.

a. Exact data, both branches of the leaky ReLU: signed dyadic data and weights for which every term of every sum of a row
   is a multiple of 2^q and sum|terms| < 2^(24 + q), so any fp32 summation order is exact; the kernel's pre-tanh value then
   equals the model's, and its output is within 2 fp32 ulp of tanh of it.  The condition is asserted on every row.
b. Random data, bars derived from the model: bf16x3 within the propagated rigorous bound (gamma(n) = n 2^-24 per sum) on
   every output and within 1e-4 of the float64 module; bf16 within gamma(n4) S4 on every DECIDED row (no hidden
   pre-activation within its gamma radius of a bf16 rounding boundary: the kernel's bf16 activations are then the model's)
   and within the old 8e-3 elsewhere.
c. Shapes (192,180,2) (188,180,2) (192,191,4) (64,100,3) (8,16,1) (4,1,3) x row counts around both workgroup sizes (128 rows
   bf16, 256 bf16x3) up to 262144 + 77.
d. Bit-exact structure: a row's action depends on nothing but the row; SWARM_POLICY_TPW=2 equals the default; bf16x3 on bf16
   rows equals bf16x3 on the same values in fp32; out= inside a larger buffer writes only its rows.
e. The exploration noise restated (helpers.policy_normals): zero weights make the action clamp(scale z).

The tests print the largest ratio of |got - model| to its derived bound and the decided fractions (pytest -s); the values
quoted in the docstrings below were measured on one MI355X.  The whole module runs in about 5 s there."""
import numpy as np
import pytest

from helpers import decided_rows, output_bound, policy_model, policy_normals, tanh_tol

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHAPES = [(192, 180, 2), (188, 180, 2), (192, 191, 4), (64, 100, 3), (8, 16, 1), (4, 1, 3)]
ROWS = [1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 4097, 262144 + 77]
PRECISIONS = ["bf16", "bf16x3"]
OLD_BF16_BAR = 8e-3          # test_gpu_policy.py's bar for rows the model cannot decide


def _fused(m, precision):
    from marl_llm_amd.rollout import FusedPolicy
    return FusedPolicy(m, precision=precision)


def _module(shape, seed, wscale=2.0, bias=0.3):
    """PolicyMLP with torch's default init, weights times wscale (so the tanh is not just its linear part), biases U(-bias,
    bias)."""
    from marl_llm_amd.rollout import PolicyMLP
    in_dim, hidden, act = shape
    torch.manual_seed(seed)
    m = PolicyMLP(in_dim, act, hidden)
    with torch.no_grad():
        for fc in (m.fc1, m.fc2, m.fc3, m.fc4):
            fc.weight.mul_(wscale); fc.bias.uniform_(-bias, bias)
    return m.cuda()


def _rows_dtype(in_dim):
    """bf16 observation rows wherever the ABI takes them (in_dim % 8 == 0)."""
    return torch.bfloat16 if in_dim % 8 == 0 else torch.float32


def _forward_at(f, x, noise_scale, seed, step, row_offset, out=None):
    """swarm_policy_forward_explore_at straight through the C ABI (FusedPolicy passes row_offset 0)."""
    rows = x.shape[0]
    out = torch.empty((rows, f.act_dim), dtype=torch.float32, device=x.device) if out is None else out
    rc = f.lib.swarm_policy_forward_explore_at(f.handle, x.data_ptr(), int(x.dtype == torch.bfloat16), rows, out.data_ptr(),
                                               float(noise_scale), seed, step, row_offset,
                                               torch.cuda.current_stream().cuda_stream)
    assert rc == 0, f.lib.swarm_policy_last_error()
    return out


def _check_against_model(got, m, x, precision, model=None):
    """The derived bars of (b) / (c).  Returns (max |got - model| / bound, decided fraction or None)."""
    mo = policy_model(m, x, precision) if model is None else model
    ref = mo["out"]
    err = (got.double() - ref).abs()
    bound = output_bound(mo, precision, m) + tanh_tol(ref)
    if precision == "bf16x3":
        assert (err <= bound).all(), "bf16x3 outside the derived bound: worst ratio %.3g" % (err / bound).max().item()
        return (err / bound).max().item(), None
    dec = decided_rows(mo)
    if dec.any():
        ratio = (err[dec] / bound[dec]).max().item()
        assert ratio <= 1.0, "bf16: a decided row is outside the derived bound (ratio %.3g)" % ratio
    else:
        ratio = 0.0
    assert err.max().item() <= OLD_BF16_BAR
    return ratio, dec.double().mean().item()


# ---------------------------------------------------------------------------------------------------------------- a. exact
def _exact_case(shape, seed, precision, n_rows):
    """Signed dyadic data for which every layer's fp32 sums are exact on every row, both leaky-ReLU branches used.

    hidden >= 8: weights {-2..2} / 16, every hidden feature's pre-activation = its bias (+B or -24 B) plus a data part
    smaller than B/2, so ~40 % of the features sit on the negative branch on every row (the leaky output 0.01 * 24 B is of
    the positive outputs' size, which keeps the terms within 24 bits of each other).  hidden < 8: zero biases, weights
    {-2..2}, each feature's sign set by the row.  Output layer scaled so that |pre-tanh| <= 2.  bf16x3 carries ~17 bits
    per activation (hi + lo of 0.01f v), so only the narrow shapes admit exact rows; rows that miss the condition are drawn
    again (rejection), and the test asserts it on every row it keeps."""
    from marl_llm_amd.rollout import PolicyMLP
    in_dim, hidden, act = shape
    g = torch.Generator().manual_seed(seed)
    m = PolicyMLP(in_dim, act, hidden).double()
    cand = 16 * n_rows if precision == "bf16x3" else n_rows + 64
    x = torch.randint(-4, 5, (cand, in_dim), generator=g).double() * 0.25
    wide = hidden >= 8
    with torch.no_grad():
        prev = x
        for li, fc in enumerate((m.fc1, m.fc2, m.fc3, m.fc4)):
            o, i = fc.weight.shape
            w = torch.randint(-2, 3, (o, i), generator=g).double() * (2.0 ** -4 if wide else 1.0)
            data = prev @ w.T
            if li == 3:
                sc = 2.0 ** torch.ceil(torch.log2(data.abs().max() / 2 + 2.0 ** -30)).item()
                w, data, b = w / sc, data / sc, torch.zeros(o, dtype=torch.float64)
            elif wide:
                B = 2.0 ** torch.ceil(torch.log2(2 * data.abs().max() + 2.0 ** -30)).item()
                neg = torch.rand(o, generator=g) < 0.4
                neg[0], neg[-1] = True, False
                b = torch.where(neg, -24.0 * B, B).double()
            else:
                b = torch.zeros(o, dtype=torch.float64)
            fc.weight.copy_(w); fc.bias.copy_(b)
            h = data + b
            prev = torch.where(h > 0, h, 0.01 * h)
    mf = m.float()
    xf = x.float()
    mo = policy_model(mf, xf, precision, device="cpu", quantum=True)
    ok = torch.ones(cand, dtype=torch.bool)
    for S, q in zip(mo["S"], mo["q"]):
        ok &= (S < 2.0 ** (24 + q[:, None])).all(dim=1)
    keep = ok.nonzero().flatten()[:n_rows]
    assert keep.numel() == n_rows, "exact generator: only %d of %d rows exact" % (ok.sum().item(), cand)
    return mf.cuda(), xf[keep]


EXACT = [("bf16", s) for s in SHAPES] + [("bf16x3", s) for s in [(4, 1, 3), (8, 2, 2), (16, 2, 4), (8, 3, 1)]]


EXACT_CASES = [(p, s, dt) for p, s in EXACT for dt in (torch.float32, torch.bfloat16) if dt == torch.float32 or s[0] % 8 == 0]


@pytest.mark.parametrize("precision,shape,dtype", EXACT_CASES,
                         ids=["%s-%d-%d-%d-%s" % ((p,) + s + ("bf16rows" if dt == torch.bfloat16 else "f32rows",))
                              for p, s, dt in EXACT_CASES])
def test_exact_data_both_leaky_branches(precision, shape, dtype):
    """Both precisions: got within 2 fp32 ulp of tanh(model) on every row, with the exactness condition asserted per row and
    per layer, and both leaky-ReLU branches present in every hidden layer (hidden >= 8: on every row; narrower: over the
    rows, for every feature).  bf16x3 only at hidden <= 3: its activations carry ~17 bits, wider layers break the
    condition."""
    in_dim, hidden, act = shape
    m, x = _exact_case(shape, 1, precision, 300)
    mo = policy_model(m, x, precision, device="cpu", quantum=True)
    for li, (S, q) in enumerate(zip(mo["S"], mo["q"])):
        assert (S < 2.0 ** (24 + q[:, None])).all(), "layer %d: a sum is not exact in fp32" % (li + 1)
    for li, h in enumerate(mo["h"][:3]):
        if hidden >= 8:
            assert ((h < 0).any(1) & (h > 0).any(1)).all(), "layer %d: a row without both branches" % (li + 1)
        else:
            assert ((h < 0).any(0) & (h > 0).any(0)).all(), "layer %d: a feature without both branches" % (li + 1)
    pre = mo["h"][3]
    assert pre.abs().max().item() <= 2.0 and pre.abs().max().item() > 0.25       # the tanh is not saturated
    got = _fused(m, precision)(x.to(dtype).cuda().contiguous()).cpu().double()
    ref = torch.tanh(pre)
    ulp = torch.from_numpy(np.spacing(ref.float().abs().numpy()).astype(np.float64))
    assert ((got - ref).abs() <= 2 * ulp).all(), "max %.3g ulp" % ((got - ref).abs() / ulp).max().item()


# ---------------------------------------------------------------------------------------------------- b. random vs model
def _low_cancellation_module(shape, seed):
    """Non-negative inputs (the observation's range), weights mostly positive and a third of each hidden layer pushed onto
    the negative branch by its bias: sums with little cancellation, so sum|terms| ~ |h| and most rows are decided.  The
    biases are full-mantissa fp32 (a bias rounded to bf16 moves h by ~2^-9 |b|)."""
    from marl_llm_amd.rollout import PolicyMLP
    in_dim, hidden, act = shape
    g = torch.Generator().manual_seed(seed)
    m = PolicyMLP(in_dim, act, hidden)
    with torch.no_grad():
        fan = in_dim
        for li, fc in enumerate((m.fc1, m.fc2, m.fc3, m.fc4)):
            o, i = fc.weight.shape
            w = torch.rand(o, i, generator=g) * (2.0 / fan)
            w[torch.rand(o, i, generator=g) < 0.15] *= -1.0
            b = torch.rand(o, generator=g) * 0.2 + 0.05
            if li < 3:
                neg = torch.rand(o, generator=g) < 0.33
                b[neg] -= 1.5
            else:                                                 # outputs of both signs, |pre-tanh| up to ~1.5
                w = (torch.rand(o, i, generator=g) * 2 - 1) * (4.0 / fan ** 0.5)
                b.zero_()
            fc.weight.copy_(w); fc.bias.copy_(b)
            fan = hidden
    return m.cuda()


LOWC = [(32, 32, 2), (64, 48, 3), (64, 64, 4), (32, 40, 1)]


@pytest.mark.parametrize("shape", LOWC, ids=["%d-%d-%d" % s for s in LOWC])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32rows", "bf16rows"])
def test_bf16_decided_rows_meet_the_derived_bound(shape, dtype):
    """bf16 on low-cancellation data at hidden 32-64 (the shapes where most rows are decided): decided rows within
    gamma(n4) S4 + tanh tolerance, the rest within 8e-3, and at least half the rows decided.  Measured (4097 rows, fp32 and
    bf16 rows alike): decided 0.904 / 0.790 / 0.671 / 0.862 for (32,32,2) / (64,48,3) / (64,64,4) / (32,40,1); worst
    |err| / bound on decided rows 0.0102.  At 180 wide with zero-mean data (test_shapes_and_row_counts) no row is decided."""
    m = _low_cancellation_module(shape, 7)
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.rand(4097, shape[0], device="cuda", generator=g).to(dtype).contiguous()
    mo = policy_model(m, x, "bf16")
    assert (mo["h"][0] < 0).any() and (mo["h"][2] < 0).any() and (mo["h"][3].abs() > 0.3).any()
    got = _fused(m, "bf16")(x)
    ratio, frac = _check_against_model(got, m, x, "bf16", mo)
    print("bf16 %s %s: decided %.3f, worst |err| / bound on decided rows %.3g" % (shape, dtype, frac, ratio))
    assert frac >= 0.5


@pytest.mark.parametrize("shape", SHAPES + LOWC, ids=["%d-%d-%d" % s for s in SHAPES + LOWC])
def test_bf16x3_meets_the_derived_bound(shape):
    """bf16x3 on random data: every output within the propagated bound, and within 1e-4 of the float64 module.  The
    propagated bound grows with the row sums of |W| and is loose at the wide shapes (about 0.7 at 192-180-2, 0.07 at 64-100-3,
    0.005 at 32-32-2); the 1e-4 bar is the sharp one there.  Measured: worst |err| / bound 0.022 (4-1-3), 1.2e-5 at 192-180-2;
    max |got - float64 module| 2.1e-5 over all shapes."""
    m = _module(shape, 21)
    g = torch.Generator(device="cuda").manual_seed(4)
    x = (torch.randn(4097, shape[0], device="cuda", generator=g) * 0.7).to(_rows_dtype(shape[0])).contiguous()
    got = _fused(m, "bf16x3")(x)
    ratio, _ = _check_against_model(got, m, x, "bf16x3")
    with torch.no_grad():
        ref64 = m.double()(x.double())
    m.float()
    d64 = (got.double() - ref64).abs().max().item()
    print("bf16x3 %s: worst |err| / bound %.3g, max |got - float64 module| %.3g" % (shape, ratio, d64))
    assert d64 <= 1e-4


# ----------------------------------------------------------------------------------------------- c. shapes x row counts
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=["%d-%d-%d" % s for s in SHAPES])
def test_shapes_and_row_counts(precision, shape):
    """Every shape at row counts on both sides of 128 and 256 up to 262144 + 77: the derived bars of (b) on every prefix,
    each call bit-identical to the same rows of the largest call.  Measured at 262221 rows: bf16 decided fraction 0 at the
    64..192-wide shapes (the 8e-3 bar applies), 0.83 at 8-16-1 and 0.99 at 4-1-3 with worst decided ratio 0.094; bf16x3
    worst ratio 0.50 (4-1-3), below 2e-4 elsewhere."""
    m = _module(shape, 5)
    g = torch.Generator(device="cuda").manual_seed(9)
    x = (torch.randn(ROWS[-1], shape[0], device="cuda", generator=g) * 0.7).to(_rows_dtype(shape[0])).contiguous()
    f = _fused(m, precision)
    full = f(x)
    mo = policy_model(m, x, precision)
    ratio, frac = _check_against_model(full, m, x, precision, mo)
    if precision == "bf16x3":
        with torch.no_grad():
            assert (full.double() - m.double()(x.double())).abs().max().item() <= 1e-4
        m.float()
    for n in ROWS[:-1]:
        got = f(x[:n])
        assert got.shape == (n, shape[2]) and torch.equal(got, full[:n]), n
    print("%s %s: worst ratio %.3g, decided %s" % (precision, shape, ratio, frac))


# ----------------------------------------------------------------------------------------------------- d. bit-exact
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32rows", "bf16rows"])
def test_a_rows_action_depends_only_on_the_row(precision, dtype):
    m = _module((192, 180, 2), 2)
    f = _fused(m, precision)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(1000, 192, device="cuda", generator=g).to(dtype).contiguous()
    ref = f(x)
    for k, n in [(0, 1), (1, 31), (7, 300), (129, 257), (999, 1), (500, 500)]:
        assert torch.equal(f(x[k:k + n].contiguous()), ref[k:k + n]), (k, n)
    for pre, post in [(1, 0), (77, 3), (128, 128), (255, 4096)]:
        big = torch.cat([torch.randn(pre, 192, device="cuda").to(dtype), x, torch.randn(post, 192, device="cuda").to(dtype)])
        assert torch.equal(f(big.contiguous())[pre:pre + 1000], ref), (pre, post)


@pytest.mark.parametrize("shape", [(192, 180, 2), (188, 180, 2), (64, 100, 3), (4, 1, 3), (192, 191, 4)],
                         ids=lambda s: "%d-%d-%d" % s)
def test_two_tiles_per_wave_equals_the_default(monkeypatch, shape):
    """SWARM_POLICY_TPW=2 (read by policy_forward on every call) gives the default's bits in bf16 mode, with and without
    noise, at row counts around its 256-row workgroup; bf16x3 ignores it."""
    m = _module(shape, 8)
    g = torch.Generator(device="cuda").manual_seed(2)
    x = (torch.randn(4097 + 300, shape[0], device="cuda", generator=g) * 0.7).to(_rows_dtype(shape[0])).contiguous()
    for precision in PRECISIONS:
        f = _fused(m, precision)
        outs = {}
        for tpw in ("1", "2"):
            monkeypatch.setenv("SWARM_POLICY_TPW", tpw)
            outs[tpw] = [f(x[:n]) for n in (1, 33, 255, 256, 257, 511, 4097 + 300)] + [f(x, noise_scale=0.2, seed=3, step=9)]
        monkeypatch.delenv("SWARM_POLICY_TPW")
        for a, b in zip(outs["1"], outs["2"]):
            assert torch.equal(a, b), (precision, a.shape)


@pytest.mark.parametrize("shape", [(192, 180, 2), (64, 100, 3), (8, 16, 1)], ids=lambda s: "%d-%d-%d" % s)
def test_bf16x3_on_bf16_rows_equals_fp32_rows_of_the_same_values(shape):
    m = _module(shape, 12)
    f = _fused(m, "bf16x3")
    xb = (torch.randn(4097, shape[0], device="cuda") * 0.8).to(torch.bfloat16).contiguous()
    assert torch.equal(f(xb), f(xb.float().contiguous()))
    assert torch.equal(f(xb, noise_scale=0.1, seed=1, step=2), f(xb.float().contiguous(), noise_scale=0.1, seed=1, step=2))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("act", [1, 3])
def test_out_inside_a_larger_buffer_writes_only_its_rows(precision, act):
    m = _module((64, 100, act), 4)
    f = _fused(m, precision)
    x = torch.randn(1000, 64, device="cuda")
    ref = f(x)
    big = torch.full((1000 + 300, act), float("nan"), device="cuda")
    for noise in (0.0, 0.3):
        big.fill_(float("nan"))
        got = f(x, out=big[129:1129], noise_scale=noise, seed=5, step=6)
        assert got.data_ptr() == big[129:].data_ptr()
        assert torch.isnan(big[:129]).all() and torch.isnan(big[1129:]).all()
        assert torch.equal(big[129:1129], ref if noise == 0.0 else f(x, noise_scale=noise, seed=5, step=6))


# ------------------------------------------------------------------------------------------------------------- e. noise
KEYS = [(0, 0, 0), (7, 3, 12345), (2 ** 64 - 1, 2 ** 63 + 5, 2 ** 40 + 3)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("act", [1, 2, 3, 4])
def test_noise_follows_the_header(precision, act):
    """All weights zero: the action is clamp(scale z) with z of include/swarm_policy.h 'Gaussian noise'.  scale = 1/8 makes
    scale z exact and keeps |scale z| < 1, so got / scale is the kernel's z, held to the restatement within 8 fp32 ulp of the
    Box-Muller radius, for fp32 and bf16 rows and several (seed, step, row_offset)."""
    from marl_llm_amd.rollout import PolicyMLP
    m = PolicyMLP(192, act, 180).cuda()
    with torch.no_grad():
        for p in m.parameters():
            p.zero_()
    f = _fused(m, precision)
    rows = 4097
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.randn(rows, 192, device="cuda").to(dtype)
        for seed, step, off in KEYS:
            got = _forward_at(f, x, 0.125, seed, step, off).cpu().double() * 8.0
            z, rad = policy_normals(seed, step, rows, act, off)
            err = (got.numpy() - z)
            assert (np.abs(err) <= rad * 2.0 ** -20 + 2.0 ** -24).all(), (seed, step, off, np.abs(err).max())


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("act", [2, 3, 4])
def test_noise_on_a_nonzero_actor_and_the_clamp(precision, act):
    """clamp(noiseless + scale z, -1, 1): within a few ulp of the restatement, exactly +-1 where the sum is clearly outside,
    at a scale where a quarter of the actions clamp."""
    m = _module((192, 180, act), 6)
    f = _fused(m, precision)
    rows = 4097
    x = torch.randn(rows, 192, device="cuda") * 0.7
    base = f(x).cpu().double().numpy()
    for scale in (0.3, 2.0):
        seed, step, off = 11, 4, 1 << 20
        got = _forward_at(f, x, scale, seed, step, off).cpu().double().numpy()
        z, rad = policy_normals(seed, step, rows, act, off)
        s = base + scale * z
        ref = np.clip(s, -1.0, 1.0)
        assert (np.abs(got - ref) <= scale * rad * 2.0 ** -20 + 2.0 ** -23 * (scale * np.abs(z) + 1)).all(), np.abs(got - ref).max()
        far = np.abs(s) > 1.0 + 1e-3
        assert (np.abs(got[far]) == 1.0).all()
        if scale == 2.0:
            assert far.mean() > 0.25
