"""The fused policy kernel's log-probability output (swarm_policy_forward_explore_logpi, include/swarm_policy.h 'Log-probability
of the noise'): exact against a numpy fp32 restatement of the header on the kernel's own normals, close to the reference's
float64 GaussianNoise.log_prob, -0.0 without noise, and no effect on the actions."""
import math

import numpy as np
import pytest

from helpers import policy_normals

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROWS = [1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 4097, 262144 + 77]
SHAPES = [(8, 16, 1), (192, 180, 2), (64, 100, 3), (192, 191, 4)]           # act_dim 1..4
SCALE = 0.125                                                               # 2^-3: act / SCALE is exact


def _zero_policy(shape, precision):
    from marl_llm_amd.rollout import FusedPolicy, PolicyMLP
    in_dim, hidden, act = shape
    m = PolicyMLP(in_dim, act, hidden).cuda()
    with torch.no_grad():
        for p in m.parameters():
            p.zero_()
    return FusedPolicy(m, precision=precision)


def _random_policy(shape, precision, seed=0):
    from marl_llm_amd.rollout import FusedPolicy, PolicyMLP
    in_dim, hidden, act = shape
    torch.manual_seed(seed)
    m = PolicyMLP(in_dim, act, hidden)
    with torch.no_grad():
        for fc in (m.fc1, m.fc2, m.fc3, m.fc4):
            fc.weight.mul_(2.0); fc.bias.uniform_(-0.3, 0.3)
    return FusedPolicy(m.cuda(), precision=precision)


def header_log_pi(z32, scale):
    """include/swarm_policy.h, restated in numpy fp32: z32 [rows, act_dim] float32 -> [rows] float32."""
    act_dim = z32.shape[1]
    c = np.float32(act_dim * math.log(float(np.float32(scale)) * math.sqrt(2.0 * math.pi)))
    s = z32[:, 0] * z32[:, 0]
    for k in range(1, act_dim):
        s = s + z32[:, k] * z32[:, k]
    return -(np.float32(0.5) * s) - c, c


def reference_log_prob(noise, scale):
    """utils/noise.py GaussianNoise.log_prob in float64."""
    lp = -0.5 * ((noise / scale) ** 2).sum(axis=-1)
    lp -= noise.shape[1] * np.log(scale * np.sqrt(2 * np.pi))
    return lp


def _dtypes(in_dim):
    return (torch.float32, torch.bfloat16) if in_dim % 8 == 0 else (torch.float32,)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
@pytest.mark.parametrize("shape", SHAPES)
def test_zero_weights_log_pi_is_the_header_formula_bit_for_bit(precision, shape, monkeypatch):
    in_dim, _, act = shape
    f = _zero_policy(shape, precision)
    seed, step, off = 7, 31, 1000
    tpws = ("1", "2") if precision == "bf16" else ("1",)
    for tpw in tpws:
        monkeypatch.setenv("SWARM_POLICY_TPW", tpw)
        for dtype in _dtypes(in_dim):
            for rows in ROWS:
                x = torch.randn(rows, in_dim, device="cuda").to(dtype)
                a, lp = f(x, noise_scale=SCALE, seed=seed, step=step, log_pi=True, row_offset=off)
                a, lp = a.cpu().numpy(), lp.cpu().numpy()
                assert a.shape == (rows, act) and lp.shape == (rows,) and lp.dtype == np.float32
                z = a / np.float32(SCALE)                                   # the kernel's own fp32 normals (exact)
                z64, rad = policy_normals(seed, step, rows, act, off)
                assert (np.abs(z - z64) <= rad * 2.0 ** -20 + 2.0 ** -24).all(), (tpw, dtype, rows)
                want, c = header_log_pi(z, SCALE)
                assert np.array_equal(_bits(lp), _bits(want)), (tpw, dtype, rows)
                ref = reference_log_prob(np.float64(SCALE) * z.astype(np.float64), SCALE)
                half = np.float32(0.5) * (z * z).sum(axis=1, dtype=np.float32)
                bound = 8 * (np.spacing(np.abs(half)) + np.spacing(np.abs(c)))       # a few fp32 ulp of both terms
                assert (np.abs(lp.astype(np.float64) - ref) <= bound).all(), (tpw, dtype, rows)
    monkeypatch.delenv("SWARM_POLICY_TPW")
    f.close()


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
@pytest.mark.parametrize("shape", [(192, 180, 2), (64, 100, 3)])
def test_log_pi_leaves_the_actions_bit_identical(precision, shape, monkeypatch):
    in_dim = shape[0]
    f = _random_policy(shape, precision)
    tpws = ("1", "2") if precision == "bf16" else ("1",)
    for tpw in tpws:
        monkeypatch.setenv("SWARM_POLICY_TPW", tpw)
        for dtype in _dtypes(in_dim):
            x = torch.randn(262144 + 77, in_dim, device="cuda").to(dtype)
            for scale, seed, step, off in ((0.1, 3, 0, 0), (0.3, 5, 77, 12345), (0.0, 1, 2, 0)):
                plain = f(x, noise_scale=scale, seed=seed, step=step, row_offset=off)
                with_lp, lp = f(x, noise_scale=scale, seed=seed, step=step, row_offset=off, log_pi=True)
                assert torch.equal(plain, with_lp), (tpw, dtype, scale)
                assert torch.isfinite(lp).all()
    monkeypatch.delenv("SWARM_POLICY_TPW")
    f.close()


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
def test_no_noise_gives_minus_zero(precision):
    f = _random_policy((192, 180, 2), precision)
    x = torch.randn(4097, 192, device="cuda")
    for scale in (0.0, -0.5):
        lp = torch.full((4097,), 3.0, device="cuda")
        _, got = f(x, noise_scale=scale, seed=1, step=2, log_pi=lp)
        assert got.data_ptr() == lp.data_ptr()
        assert (got == 0).all() and torch.signbit(got).all()
    f.close()


def test_row_offset_shards_the_log_pi_of_a_whole_batch_call():
    f = _random_policy((192, 180, 2), "bf16")
    x = torch.randn(1000, 192, device="cuda")
    _, full = f(x, noise_scale=0.2, seed=4, step=6, log_pi=True)
    _, lo = f(x[:400], noise_scale=0.2, seed=4, step=6, log_pi=True)
    _, hi = f(x[400:], noise_scale=0.2, seed=4, step=6, log_pi=True, row_offset=400)
    assert torch.equal(full, torch.cat([lo, hi]))
    f.close()


def test_bad_log_pi_arguments_are_rejected():
    f = _random_policy((192, 180, 2), "bf16")
    x = torch.randn(64, 192, device="cuda")
    for bad in (torch.empty(63, device="cuda"), torch.empty(64, device="cuda", dtype=torch.float64), torch.empty(64),
                torch.empty(128, device="cuda")[::2], "yes"):
        with pytest.raises(ValueError):
            f(x, noise_scale=0.1, log_pi=bad)
    assert isinstance(f(x, noise_scale=0.1), torch.Tensor)                  # without log_pi: the actions alone, as before
    f.close()
