"""Host-side pieces of bench.py that need no GPU: the CPU-baseline worker pool (independent processes stepping the
reference's CPU path over their own envs) and the SURVEY 8(d) byte accounting."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_cpu_worker_pool(tmp_path, shapes, oracle):
    import bench
    from marl_llm_amd.shapes import r_avoid_for
    from marl_llm_amd.synth import synthetic_batch
    E, N = 6, 16
    ra = r_avoid_for(N, shapes)
    sy = synthetic_batch(E, N, shapes, seed=1, assembled_fraction=0.5)
    nei = np.stack([oracle.get_observation(sy["p"][e], sy["dp"][e], sy["cells"][e][:, : sy["n_g"][e]],
                                           float(sy["l_cell"][e]), ra)["neighbor_index"] for e in range(E)])
    path = str(tmp_path / "state.npz")
    np.savez(path, p=sy["p"], dp=sy["dp"], nei=nei, cells=sy["cells"], n_g=sy["n_g"], l_cell=sy["l_cell"])
    pool = bench.start_cpu_workers(2)
    r = bench.run_cpu_leg(pool, path, N, ra, budget_s=1.0, steps_per_env=5)
    assert r["value"] > 0 and 2 <= r["envs"] <= E and r["kind"] in ("reference", "port")
    assert all(p.returncode == 0 for p in pool)


def test_survey_bytes_matches_section_8d():
    import bench
    # N = 64, n_g = 512 -> 885 B per agent-step
    b = bench.survey_bytes(64, np.full(4096, 512))
    assert b == 4096 * 64 * (821 + 8 * 512 / 64) and abs(b / (4096 * 64) - 885) < 1e-9
    assert bench.host_cores() >= 1


class _FakeBatch:
    """The part of SwarmBatch that bench.dump_outputs reads, on CPU tensors."""

    def __init__(self, E, N, D, seed):
        import torch
        g = torch.Generator().manual_seed(seed)
        self.n_env, self.n_agents, self.obs_dim, self.device = E, N, D, torch.device("cpu")
        self.p = torch.rand((E, 2, N), generator=g, dtype=torch.float64)
        self.dp = torch.rand((E, 2, N), generator=g, dtype=torch.float64)
        self.last = (torch.rand((E, N, D), generator=g), torch.rand((E, N), generator=g),
                     (torch.rand((E, N), generator=g) < 0.5).to(torch.uint8), torch.rand((E, N, 2), generator=g))

    def get_state(self):
        return self.p, self.dp


def test_dump_outputs_rows_dtypes_and_size_cap(tmp_path, monkeypatch):
    """bench.py --dump-outputs: one row per agent (env-major), float32 / float64 only, every row while they fit, else the
    same fixed sample of rows in every array and in every run, within DUMP_BYTES."""
    import torch
    import bench
    E, N, D = 5, 8, 192
    sb = _FakeBatch(E, N, D, seed=0)
    bench.dump_outputs(torch, str(tmp_path / "all"), sb, sb.last)
    z = {f[:-4]: np.load(str(tmp_path / "all" / f)) for f in os.listdir(tmp_path / "all")}
    assert sorted(z) == ["a_prior", "done", "dp", "obs", "p", "reward", "rows"]
    assert all(a.dtype in (np.float32, np.float64) for a in z.values())
    assert z["p"].dtype == z["dp"].dtype == np.float64
    assert np.array_equal(z["rows"], np.arange(E * N))
    obs, rew, done, pri = (t.numpy() for t in sb.last)
    assert np.array_equal(z["obs"], obs.reshape(E * N, D)) and np.array_equal(z["reward"], rew.reshape(-1))
    assert np.array_equal(z["done"], done.reshape(-1).astype(np.float32)) and np.array_equal(z["a_prior"], pri.reshape(-1, 2))
    assert np.array_equal(z["p"], sb.p.numpy().transpose(0, 2, 1).reshape(-1, 2))
    assert np.array_equal(z["dp"], sb.dp.numpy().transpose(0, 2, 1).reshape(-1, 2))

    monkeypatch.setattr(bench, "DUMP_BYTES", 16 * 1024)
    for name, seed in (("a", 1), ("b", 2)):
        sb = _FakeBatch(E, N, D, seed)
        bench.dump_outputs(torch, str(tmp_path / name), sb, sb.last)
    za, zb = ({f[:-4]: np.load(str(tmp_path / d / f)) for f in os.listdir(tmp_path / d)} for d in ("a", "b"))
    rows = za["rows"].astype(np.int64)
    assert np.array_equal(za["rows"], zb["rows"]) and 0 < len(rows) < E * N and (np.diff(rows) > 0).all()
    assert sum(a.nbytes for a in za.values()) <= 16 * 1024
    obs = sb.last[0].numpy().reshape(E * N, D)
    assert np.array_equal(zb["obs"], obs[rows]) and np.array_equal(zb["p"], sb.p.numpy().transpose(0, 2, 1).reshape(-1, 2)[rows])
