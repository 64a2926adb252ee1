"""The one comparison of the HIP env step with the oracle, for every test that holds the step to it.

The contract (include/swarm_env.h): every output of a step -- state, observation, prior, reward, done and the four index
lists -- is bit for bit what the oracle gives from the same state; obs / a_prior as helpers.as_obs_dtype rounds the oracle's
double to the handle's obs dtype.  device_layout puts an oracle result into the device's layout, host_copy copies a handle's
outputs to the host, compare holds one to the other and names the field, the call and the envs that differ, hold runs a
whole recorded trajectory through a fresh handle, and Lockstep runs a handle and the threaded oracle side by side.
tests/test_lockstep_host.py checks on the CPU that compare catches one changed element of every field.
"""
import os

import numpy as np

from helpers import ThreadedOracle, as_obs_dtype, pad_cells

IDX = ("neighbor_index", "in_flags", "sensed_index", "occupied_index")
OBSERVE = ("obs",) + IDX + ("unused",)                  # what observe() gives
OUTPUTS = ("obs", "a_prior", "reward", "done")
FIELDS = ("p", "dp") + OUTPUTS + IDX + ("unused",)      # what a step gives; "unused": the unused sensed slots of obs are zero
SIZE_A = 0.035


class Mismatch(AssertionError):
    """A field of the device's outputs differs from the oracle's: .field, .tag (the caller's, e.g. the step number) and
    .envs (the envs that differ, offset by the caller's env0)."""

    def __init__(self, field, tag, envs, why=""):
        envs = np.asarray(envs)
        super().__init__(f"{tag}: {field}: {why or '%d env(s) differ, first %s' % (len(envs), list(envs[:8]))}")
        self.field, self.tag, self.envs = field, tag, envs


def dtype_name(sb):
    """helpers.as_obs_dtype's name of a handle's obs dtype."""
    return {"torch.float64": "f64", "torch.float32": "f32", "torch.bfloat16": "bf16"}[str(sb.obs_dtype)]


def device_layout(o, dtype="f64"):
    """An oracle result in the device's layout and dtype.  o: [E] per-env dicts of oracle.get_observation / oracle.step /
    helpers.oracle_run, or ThreadedOracle's dict of [E, ...] arrays.  obs [E, D, N] -> [E, N, D] and a_prior [E, 2, N] ->
    [E, N, 2], both as a handle of `dtype` ("f64", "f32", "bf16") returns them; reward [E, N] float64; the rest stacked."""
    if not isinstance(o, dict):
        o = {k: np.stack([r[k] for r in o]) for k in o[0] if o[0][k] is not None}
    out = dict(o)
    for k in ("obs", "a_prior"):
        if o.get(k) is not None:
            out[k] = np.ascontiguousarray(np.swapaxes(as_obs_dtype(o[k], dtype), 1, 2))       # rounded where it lies, then laid out
    if "reward" in o:
        out["reward"] = np.asarray(o["reward"], np.float64).reshape(len(o["reward"]), -1)
    return out


def to_host(t):
    """A device tensor as numpy, bfloat16 widened exactly to float32."""
    return (t.float() if str(t.dtype) == "torch.bfloat16" else t).cpu().numpy()


def oracle_action(act):
    """A device action [E, N, 2] (tensor or array, float32 or float64) as ThreadedOracle.step takes it: [E, 2, N] float64, exact."""
    return np.swapaxes(act if isinstance(act, np.ndarray) else to_host(act), 1, 2).astype(np.float64)


def host_copy(sb, out, state=True, indices=False, rows=slice(None)):
    """Host copies of a handle's outputs.  out: what sb.step returned (obs, reward, done, a_prior), the dict a caller passed
    as step's `out`, or sb.observe()'s tensor.  state: p and dp too (one get_state call; or the (p, dp) tensors to copy).
    indices: the four index arrays too -- sb.indices() runs the observation pass again, so long runs ask for it rarely (or
    pass the dict of tensors they already hold).  rows: the envs to copy.  "head" is the width of obs before the sensed
    slots, 4 (topo + 1 + with_self)."""
    if isinstance(out, dict):
        out = (out["obs"], out["rew"], out["done"], out["prior"])
    names = ("obs", "reward", "done", "a_prior") if isinstance(out, tuple) else ("obs",)
    dev = {k: to_host(t[rows]) for k, t in zip(names, out if isinstance(out, tuple) else (out,)) if t is not None}      # no prior: None
    if "reward" in dev:
        dev["reward"] = dev["reward"].astype(np.float64)
    if state:
        dev["p"], dev["dp"] = [to_host(t[rows]) for t in (sb.get_state() if state is True else state)]
    if indices:
        dev.update({k: to_host(t[rows]) for k, t in (sb.indices() if indices is True else indices).items()})
    dev["head"] = sb.obs_dim - 2 * sb.g_max
    return dev


def compare(dev, ref, tag="", *, fields=FIELDS, indices=True, envs=None, env0=0):
    """Hold the device's outputs `dev` (host_copy) to the oracle's `ref` (device_layout): exact equality of every field of
    `fields`, done == 0, and obs exactly zero in the sensed slots where the device's sensed_index < 0.  indices=False leaves
    out the four index lists and the unused-slot rule (a step whose indices were not exported).  envs: the envs of dev that
    the rows of ref are the oracle's results for (default: all, in order).  Raises Mismatch naming the first field that
    differs and its envs, as numbered in dev plus env0."""
    sel = slice(None) if envs is None else np.asarray(envs)
    envs = np.arange(len(dev["obs"]))[sel]
    for f in fields:
        if not indices and (f in IDX or f == "unused"):
            continue
        if f == "unused":
            slots = dev["obs"][sel][:, :, dev["head"]:]                       # (x, y) per sensed slot
            diff = ((slots[:, :, 0::2] != 0) | (slots[:, :, 1::2] != 0)) & (dev["sensed_index"][sel] < 0)
            diff = diff if diff.any() else None
        elif f == "done":
            diff = dev[f][sel] != 0 if dev[f][sel].any() else None
        elif dev[f][sel].shape != ref[f].shape:
            raise Mismatch(f, tag, envs + env0, f"shape {dev[f][sel].shape} against the oracle's {ref[f].shape}")
        else:
            diff = None if np.array_equal(dev[f][sel], ref[f]) else dev[f][sel] != ref[f]
        if diff is not None:                   # the common case costs one pass; which envs differ is worked out only now
            raise Mismatch(f, tag, envs[diff.reshape(len(diff), -1).any(axis=1)] + env0)


def hold(cases, ref, *, lattice=None, paths=None, fields=FIELDS, pad=3, **kw):
    """Run `cases` [(p, dp, grid, l_cell)] through a fresh SwarmBatch(**kw) and hold every call to `ref` = (first, steps, ...)
    as helpers.oracle_run returns it: cells padded by `pad` and uploaded, lattice_envs() == lattice and path_envs() == paths
    (before the first and after the last call) if given, set_state and observe compared, then one step per entry of `steps`
    with the action recorded under "act", all of `fields` compared after each (tag: "observe", then the step number).  Returns the index arrays of every call, with p, dp and reward for the
    steps."""
    from marl_llm_amd.batched import SwarmBatch
    import torch
    first, steps = ref[0], ref[1]
    cells, n_g = pad_cells([c[2] for c in cases], max(c[2].shape[1] for c in cases) + pad)
    sb = SwarmBatch(n_env=len(cases), n_agents=cases[0][0].shape[1], n_cells_max=cells.shape[2], **kw)
    dtype = dtype_name(sb)
    seen = []
    try:
        sb.set_cells(cells, n_g, [c[3] for c in cases])
        if lattice is not None:
            assert sb.lattice_envs() == lattice, (sb.lattice_envs(), lattice)
        if paths is not None:
            assert sb.path_envs() == tuple(paths), (sb.path_envs(), paths)
        sb.set_state(np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]))
        dev = host_copy(sb, sb.observe(), state=False, indices=True)
        compare(dev, device_layout(first, dtype), "observe", fields=[f for f in OBSERVE if f in fields])
        seen.append({k: dev[k] for k in IDX})
        for t, step in enumerate(steps):
            want = device_layout(step, dtype)
            dev = host_copy(sb, sb.step(torch.from_numpy(want["act"]).to(sb.device)), indices=True)
            compare(dev, want, t, fields=fields)
            seen.append({k: dev[k] for k in IDX + ("p", "dp", "reward")})
        if paths is not None:
            assert sb.path_envs() == tuple(paths), (sb.path_envs(), paths)
    finally:
        sb.close()
    return seen


def dump(tag, t, e, pre, to, flags):
    """With SWARM_PARITY_DUMP=<dir> set: env e's pre-step inputs to <dir>/<tag>_t<t>_e<e>.npz, for arbitration on the CPU."""
    d = os.environ.get("SWARM_PARITY_DUMP")
    if not d:
        return
    os.makedirs(d, exist_ok=True)
    np.savez(os.path.join(d, f"{tag}_t{t}_e{e}.npz"), p=pre["p"][e], dp=pre["dp"][e], neighbor_index=pre["nei"][e],
             action=pre["a"][e], cells=to.cells[e][:, : to.n_g[e]], n_g=to.n_g[e], l_cell=to.l_cell[e],
             r_avoid=to.r_avoid, is_boundary=to.is_boundary, with_self=to.with_self, debug_flags=flags)


class Lockstep:
    """A SwarmBatch and the threaded oracle run side by side from the same state, prior-policy actions.  The four index
    arrays are compared every idx_every steps and on the last step of a run."""

    def __init__(self, oracle, sb, sy, ra, tag, is_boundary=True, with_self=True, flags=0, idx_every=25):
        import torch
        self.sb, self.tag, self.flags, self.idx_every = sb, tag, flags, idx_every
        self.dtype = dtype_name(sb)
        self.to = ThreadedOracle(oracle, sy["cells"], sy["n_g"], sy["l_cell"], ra, is_boundary=is_boundary, with_self=with_self)
        self.p, self.dp = sy["p"].copy(), sy["dp"].copy()
        self.act = torch.zeros((sb.n_env, sb.n_agents, 2), dtype=torch.float32, device=sb.device)    # bench: zero first action
        self.t = 0
        self.max_contacts = 0          # most colliding pairs (centre distance < 2 size_a) seen in any one step
        self.nei = None
        self.observe()

    def observe(self):
        """sb.observe() (needed after set_state / set_cells) against the oracle's observation of the same state."""
        dev = host_copy(self.sb, self.sb.observe(), state=False, indices=True)
        o = self.to.observe(self.p, self.dp)
        compare(dev, device_layout(o, self.dtype), f"{self.tag} observe t={self.t}", fields=OBSERVE)
        if self.nei is not None and not np.array_equal(o["neighbor_index"], self.nei):
            raise AssertionError(f"{self.tag} observe t={self.t}: neighbor_index is not the last step's")      # agents only
        self.nei = o["neighbor_index"]
        self.act = self.act.clone()    # the step writes its prior into a ping-pong buffer that observe() has shifted

    def set_cells(self, cells, n_g, l_cell, env_begin):
        self.sb.set_cells(cells, n_g, l_cell, env_begin=env_begin)
        c = self.to.cells.copy(); g = self.to.n_g.copy(); lc = self.to.l_cell.copy()
        c[env_begin: env_begin + len(n_g)] = cells; g[env_begin: env_begin + len(n_g)] = n_g
        lc[env_begin: env_begin + len(n_g)] = l_cell
        self.to.set_cells(c, g, lc)

    def run(self, steps):
        for s in range(steps):
            self.t += 1
            a = oracle_action(self.act)
            pre = dict(p=self.p, dp=self.dp, nei=self.nei, a=a)
            out = self.sb.step(self.act)
            o = self.to.step(self.p, self.dp, a, self.nei)
            with_idx = self.t % self.idx_every == 0 or s == steps - 1
            try:
                compare(host_copy(self.sb, out, indices=with_idx), device_layout(o, self.dtype), f"{self.tag} step {self.t}",
                        indices=with_idx)
            except Mismatch as ex:
                dump(self.tag, self.t, int(ex.envs[0]), pre, self.to, self.flags)
                raise
            self.p, self.dp, self.nei = o["p"], o["dp"], o["neighbor_index"]
            self.act = out[3]
            if self.to.is_boundary:
                d = self.p[:, :, :, None] - self.p[:, :, None, :]
                dc = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2)
                self.max_contacts = max(self.max_contacts, int(((dc < 2 * SIZE_A).sum() - dc[..., 0].size) // 2))
            self.last = o

    def close(self):
        self.to.close()
        self.sb.close()
