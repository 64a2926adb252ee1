"""Device-resident rollout loop.

The reference rolls out on the host: `torch.Tensor(obs)` -> policy MLP on the CPU -> numpy actions -> `env.step` -> numpy
ring buffer (train_assembly.py:91-111, maddpg.py:72-87, agents.py:69-96, buffer_agent.py:67-128).  Once the env emits
`[E, N, D]` device tensors that round trip is the bottleneck, so this module keeps the whole transition on the GPU:

* `PolicyMLP`     -- the reference's actor shape (networks.py:6-44: 4 x Linear, leaky-ReLU, tanh out) as a plain torch
                     module (the learner trains this one).
* `FusedPolicy`   -- the same forward as one hand-written bf16-MFMA kernel (csrc/policy_mlp.hip) for the rollout.
* `FusedPolicyBank` -- M actors of one shape in one handle and one launch: env group m of a batch acts with member m
                     (checkpoints of a run, seeds of a sweep, a population of learners); a FusedPolicy to every loop below.
                     `assign(member_of_env, N)` routes it by env instead: a device table names each env's member.
* `DeviceReplay`  -- the ring buffer of buffer_agent.py:13-128 with one row per (env, agent) transition, as device tensors.
* `ChainedReplay` -- the same transitions stored as a ring of env steps that share observation rows (half the copy per push).
* `rollout`       -- obs -> policy -> exploration noise (agents.py:82-96 continuous branch) -> env.step_tensor -> push.
* `rollout_device`-- the same loop (fused policy, chained ring) as ONE library call per episode: swarm_rollout; with
                     log_pi=True also each action's log-probability (swarm_rollout_logpi), the AIRL agent side's log_pi;
                     with coin="env" the epsilon coin and the noise scale per env, drawn on the device (swarm_rollout_explore).
* `rollout_expert`-- expert rollouts (rule-based expert or the prior's 'llm' twin) into the same ring, one library call per
                     episode batch: swarm_rollout_expert (collect_expert_data.py's loop on the device).
* `EpisodeClock`  -- staggered episodes for the device loops: the resets= schedule (whole-batch and per-env resets inside a
                     call, SwarmBatch.reset_envs) that keeps the envs of a batch out of phase.
* `save_expert_data` -- a ring's transitions as the expert_data.npz that ReplayBufferExpert.load reads (train_assembly_airl.py).
* `rollout_eval`  -- evaluation rollouts (eval_assembly.py's loop on the device), one library call: swarm_rollout_eval -- the
                     actor without noise, per step the three wrapper metrics of every env, a state trace and target-shape
                     switches that never return to the host.
* `save_eval_results` -- a rollout_eval trace as the metrics.pkl / state_data.npz eval_assembly.py writes, plus the batch's
                     per-step mean / std over envs.

PyTorch is plumbing here (device memory, GEMMs); the environment step is the HIP library.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


class PolicyMLP(nn.Module):
    def __init__(self, obs_dim=192, act_dim=2, hidden_dim=180):          # assembly_cfg.py:185 hidden_dim = 180
        super().__init__()
        self.fc1 = nn.Linear(obs_dim, hidden_dim)
        self.fc2 = nn.Linear(hidden_dim, hidden_dim)
        self.fc3 = nn.Linear(hidden_dim, hidden_dim)
        self.fc4 = nn.Linear(hidden_dim, act_dim)

    def forward(self, x):
        h = F.leaky_relu(self.fc1(x))
        h = F.leaky_relu(self.fc2(h))
        h = F.leaky_relu(self.fc3(h))
        return torch.tanh(self.fc4(h))


class FusedPolicy:
    """The same actor evaluated by ONE hand-written HIP kernel (csrc/policy_mlp.hip: bf16 MFMA, fp32 accumulate, the four
    layers chained through the accumulator registers) instead of four hipBLASLt GEMMs + elementwise kernels.  Inference
    only (rollouts); numerics = torch.autocast(bfloat16) on the module.  Built from a PolicyMLP (or any module with
    fc1..fc4); after the learner updated the weights call `sync()` (device parameters, in stream order, no host wait) or
    `refresh()` (a new handle from a host copy; blocks).  No CPU path.

    Two geometries of the kernel: the narrow one (in_dim <= 192, hidden <= 191: the reference's default shapes) and the wide
    one (csrc/policy_wide.hip: in_dim <= 384, hidden <= 256 -- `--hidden_dim` up to 256, `num_obs_grid_max` up to 176 at the
    default topology).  `.wide` says which one the handle runs."""

    def __init__(self, module, device="cuda:0", precision="bf16", wide=None):
        """precision: "bf16" (operands rounded to bfloat16: torch.autocast's contract, ~4e-2 from the fp32 module) or "bf16x3"
        (high + low bfloat16 parts, three MFMAs per product: ~1e-4 from the fp32 module, the reference's actor arithmetic
        for rollouts that must follow networks.py:6-44 closely).
        wide: None -- the narrow kernel where it serves the module's shape, the wide one otherwise; True -- the wide kernel
        always; False -- the narrow kernel, or its error."""
        import ctypes
        if precision not in ("bf16", "bf16x3"):
            raise ValueError("precision must be 'bf16' or 'bf16x3'")
        self.precision = precision
        self._want_wide = wide
        self.wide = bool(wide)
        from . import _lib
        self._ctypes = ctypes
        self.lib = _lib.load()
        self.module = module
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("FusedPolicy needs a cuda (HIP) device; there is no CPU path")
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self.handle = None
        self.refresh()

    def refresh(self):
        ct = self._ctypes
        m = self.module
        ws = [t.detach().to("cpu", torch.float32).contiguous() for t in
              (m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, m.fc3.weight, m.fc3.bias, m.fc4.weight, m.fc4.bias)]
        self.in_dim, self.hidden, self.act_dim = ws[0].shape[1], ws[0].shape[0], ws[6].shape[0]
        h = ct.c_void_p()
        narrow_serves = 4 <= self.in_dim <= 192 and self.in_dim % 4 == 0 and 1 <= self.hidden <= 191 and 1 <= self.act_dim <= 4
        wide = (not narrow_serves) if self._want_wide is None else bool(self._want_wide)
        name = "swarm_policy_create_wide" if wide else "swarm_policy_create"
        rc = getattr(self.lib, name)(*[ct.c_void_p(w.data_ptr()) for w in ws], self.in_dim, self.hidden, self.act_dim,
                                     self.device.index, ct.byref(h))
        if rc != 0:
            raise RuntimeError(name + " failed: " + self.lib.swarm_policy_last_error().decode())
        self.wide = wide
        self.close()
        self.handle = h
        if self.lib.swarm_policy_set_precision(self.handle, 1 if self.precision == "bf16x3" else 0) != 0:
            raise RuntimeError("swarm_policy_set_precision failed: " + self.lib.swarm_policy_last_error().decode())

    def sync(self):
        """Load the module's current parameters into the existing handle, in stream order (swarm_policy_load_device,
        include/swarm_policy.h): one packing kernel enqueued on torch's current stream of the device, the stream `__call__`
        uses.  Enqueue only -- no host synchronisation, no allocation in the library, nothing goes through the host: a
        forward or rollout enqueued before the call uses the old weights, one enqueued after it the new ones, and the
        parameters are read when the kernel runs (in-place updates enqueued on that stream before sync() are seen).
        The packed weights are byte for byte those of `refresh()`.  A parameter that is float32, contiguous and on the
        device is read in place; another dtype or layout is converted on the device first.  The parameters must be on the
        policy's device and of the shapes the handle was built with: otherwise ValueError, before any library call -- use
        `refresh()`, which takes host weights and new shapes."""
        ct = self._ctypes
        m = self.module
        ps = [m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, m.fc3.weight, m.fc3.bias, m.fc4.weight, m.fc4.bias]
        want = [(self.hidden, self.in_dim), (self.hidden,), (self.hidden, self.hidden), (self.hidden,),
                (self.hidden, self.hidden), (self.hidden,), (self.act_dim, self.hidden), (self.act_dim,)]
        if any(tuple(t.shape) != w for t, w in zip(ps, want)):
            raise ValueError("sync(): the module's (in_dim, hidden, act_dim) are not the handle's (%d, %d, %d); refresh() builds "
                             "a handle for new shapes" % (self.in_dim, self.hidden, self.act_dim))
        if any(t.device != self.device for t in ps):
            raise ValueError("sync() reads the parameters on %s; refresh() loads parameters kept on another device" % (self.device,))
        # a conversion runs on the current stream of the device, where the kernel goes; the caching allocator hands the staging
        # tensor's memory to later work of that stream only, so it may be dropped on return
        ws = [t.detach() if t.dtype == torch.float32 and t.is_contiguous() else t.detach().to(torch.float32).contiguous()
              for t in ps]
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self.lib.swarm_policy_load_device(self.handle, *[ct.c_void_p(w.data_ptr()) for w in ws], ct.c_void_p(stream))
        if rc != 0:
            raise RuntimeError("swarm_policy_load_device failed: " + self.lib.swarm_policy_last_error().decode())

    def __call__(self, obs, out=None, noise_scale=0.0, seed=0, step=0, log_pi=None, row_offset=0):
        """obs [rows, in_dim] float32 or bfloat16 on the device (contiguous) -> actions [rows, act_dim] float32.
        noise_scale > 0: the exploring actor of agents.py:93-96 in the same launch -- clamp(action + noise_scale * N(0, 1),
        -1, 1) with a counter-based generator keyed by (seed, step, row_offset + row).  out: where to write (a contiguous
        float32 tensor of rows * act_dim elements, e.g. a replay-ring slot).
        log_pi: a contiguous float32 tensor of `rows` elements on the device, or True to allocate one -- the kernel also
        writes each row's log-probability of its noise (GaussianNoise.log_prob, include/swarm_policy.h; -0.0 without
        noise) and the call returns (actions, log_pi [rows]).  The actions are the same bits either way."""
        if (obs.dtype not in (torch.float32, torch.bfloat16) or not obs.is_contiguous() or obs.device != self.device
                or obs.shape[-1] != self.in_dim):
            raise ValueError("FusedPolicy expects a contiguous float32 / bfloat16 [rows, %d] tensor on %s" % (self.in_dim, self.device))
        rows = obs.numel() // self.in_dim
        if out is None:
            out = torch.empty((rows, self.act_dim), dtype=torch.float32, device=self.device)
        elif (out.dtype != torch.float32 or out.device != self.device or not out.is_contiguous() or out.numel() != rows * self.act_dim):
            raise ValueError("out must be a contiguous float32 tensor of %d elements on %s" % (rows * self.act_dim, self.device))
        if log_pi is True:
            log_pi = torch.empty(rows, dtype=torch.float32, device=self.device)
        elif log_pi is not None and (not isinstance(log_pi, torch.Tensor) or log_pi.dtype != torch.float32 or log_pi.device != self.device
                                     or not log_pi.is_contiguous() or log_pi.numel() != rows):
            raise ValueError("log_pi must be True or a contiguous float32 tensor of %d elements on %s" % (rows, self.device))
        stream = torch.cuda.current_stream(self.device).cuda_stream
        m64 = 2 ** 64 - 1
        args = (float(noise_scale), int(seed) & m64, int(step) & m64, int(row_offset) & m64, stream)
        if log_pi is None:
            rc = self.lib.swarm_policy_forward_explore_at(self.handle, obs.data_ptr(), int(obs.dtype == torch.bfloat16), rows,
                                                          out.data_ptr(), *args)
        else:
            rc = self.lib.swarm_policy_forward_explore_logpi(self.handle, obs.data_ptr(), int(obs.dtype == torch.bfloat16), rows,
                                                             out.data_ptr(), log_pi.data_ptr(), *args)
        if rc != 0:
            raise RuntimeError("swarm_policy_forward failed: " + self.lib.swarm_policy_last_error().decode())
        act = out.view(rows, self.act_dim)
        return act if log_pi is None else (act, log_pi.view(rows))

    def close(self):
        if self.handle is not None:
            self.lib.swarm_policy_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _fc_params(m):
    return (m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, m.fc3.weight, m.fc3.bias, m.fc4.weight, m.fc4.bias)


def _bank_shape(modules):
    """(in_dim, hidden, act_dim) shared by the modules of a bank; ValueError where they differ (no library call)."""
    if len(modules) < 1:
        raise ValueError("FusedPolicyBank needs at least one module")
    shapes = [[tuple(t.shape) for t in _fc_params(m)] for m in modules]
    in_dim, hidden, act_dim = shapes[0][0][1], shapes[0][0][0], shapes[0][6][0]
    want = [(hidden, in_dim), (hidden,), (hidden, hidden), (hidden,), (hidden, hidden), (hidden,), (act_dim, hidden), (act_dim,)]
    for k, s in enumerate(shapes):
        if s != want:
            raise ValueError("FusedPolicyBank: module %d has parameter shapes %s; a bank's members share one shape, (in_dim, "
                             "hidden, act_dim) = (%d, %d, %d) of module 0" % (k, s, in_dim, hidden, act_dim))
    return in_dim, hidden, act_dim


class FusedPolicyBank(FusedPolicy):
    """M actors of one shape in ONE handle and one launch per forward (swarm_policy_bank_create, include/swarm_policy.h): over
    `rows` rows, member m evaluates the contiguous rows [m R, (m + 1) R), R = rows / M -- in a rollout the envs
    [m E / M, (m + 1) E / M).  Every row gets the bits a plain FusedPolicy of its member's module gives it (actions and
    log_pi; the noise is keyed by row_offset + row as ever).  A FusedPolicy to `rollout`, `rollout_device` and `rollout_eval`:
    they take it unchanged, and refuse E % M != 0.

    modules: the members, each with fc1..fc4 of the same shapes (ValueError otherwise, before any library call).
    precision, wide: as FusedPolicy, for all members; wide=None picks the geometry by FusedPolicy's rule.
    `.members` = M, `.modules` the list; `refresh()` builds a new handle from host copies of all members; `sync(member=None)`
    loads the device parameters of one member, or of all (one packing launch each), in stream order.

    Routing by env (swarm_policy_bank_route): `assign(member_of_env, rows_per_env)` puts a table in force that names the member
    of every env -- unequal groups, any order, -1 for an env nobody serves, E % M free; `assign(None)` ends it.  The loops take
    the routed bank unchanged; `routing()` reads back what the routing kernel built."""

    def __init__(self, modules, device="cuda:0", precision="bf16", wide=None):
        self.modules = list(modules)
        self.members = len(self.modules)
        self._route = None              # (int32 device table [E], rows_per_env) of the assignment in force
        _bank_shape(self.modules)
        super().__init__(self.modules[0], device=device, precision=precision, wide=wide)

    def refresh(self):
        ct = self._ctypes
        self.in_dim, self.hidden, self.act_dim = _bank_shape(self.modules)
        ws = [t.detach().to("cpu", torch.float32).contiguous() for m in self.modules for t in _fc_params(m)]
        narrow_serves = 4 <= self.in_dim <= 192 and self.in_dim % 4 == 0 and 1 <= self.hidden <= 191 and 1 <= self.act_dim <= 4
        wide = (not narrow_serves) if self._want_wide is None else bool(self._want_wide)
        table = (ct.c_void_p * len(ws))(*[w.data_ptr() for w in ws])
        h = ct.c_void_p()
        rc = self.lib.swarm_policy_bank_create(table, self.members, self.in_dim, self.hidden, self.act_dim, int(wide),
                                               self.device.index, ct.byref(h))
        if rc != 0:
            raise RuntimeError("swarm_policy_bank_create failed: " + self.lib.swarm_policy_last_error().decode())
        self.wide = wide
        self.close()
        self.handle = h
        if self.lib.swarm_policy_set_precision(self.handle, 1 if self.precision == "bf16x3" else 0) != 0:
            raise RuntimeError("swarm_policy_set_precision failed: " + self.lib.swarm_policy_last_error().decode())
        if self._route is not None:                           # the assignment in force, for the new handle
            self._enqueue_route(*self._route)

    def _enqueue_route(self, table, rows_per_env):
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self.lib.swarm_policy_bank_route(self.handle, self._ctypes.c_void_p(table.data_ptr()), int(table.numel()), int(rows_per_env),
                                              self._ctypes.c_void_p(stream))
        if rc != 0:
            if rc == 2:                                       # a HIP error ends the route in the library (swarm_policy.h)
                self._route = None
            raise RuntimeError("swarm_policy_bank_route failed: " + self.lib.swarm_policy_last_error().decode())

    def assign(self, member_of_env, rows_per_env=None, n_env=None):
        """Route the bank by env (swarm_policy_bank_route, include/swarm_policy.h): env e acts with member member_of_env[e],
        every env being `rows_per_env` consecutive rows (the env's agents N).  The route goes on torch's current stream: a
        forward or rollout enqueued before the call uses the previous assignment, one enqueued after it the new one.
        With a DEVICE table the call is enqueue only (after the first assignment, which allocates).  With a HOST array it is
        not: the copy of the array to the device is a pageable-memory copy on that stream, and the host waits in it for the
        work the stream still holds -- re-assign from a device table where the host must not stall.
        member_of_env:
          * a host int array / sequence [E], entries in [-1, M) (-1: an env nobody serves -- its action rows are not written):
            checked here (ValueError before any library call), then copied into an int32 device tensor the bank owns;
          * a contiguous int32 cuda tensor [E] on the bank's device: used as it is, read when the routing kernel runs (writes
            enqueued on the stream before are seen; entries outside [0, M) are unserved) and not read again afterwards: the
            caller keeps it alive until then, and rewriting it later changes nothing until the next assign() -- or refresh(),
            which routes the new handle from what the tensor then holds;
          * None: ends the route -- equal contiguous groups again.
        n_env (optional): the E the caller expects -- the env batch's -- so that a table of another length is a ValueError
        here and not a refusal of the next rollout.  Anything else: ValueError."""
        if member_of_env is None:
            rc = self.lib.swarm_policy_bank_route(self.handle, None, 0, 0, None)
            if rc != 0:
                raise RuntimeError("swarm_policy_bank_route failed: " + self.lib.swarm_policy_last_error().decode())
            self._route = None
            return
        if rows_per_env is None or int(rows_per_env) != rows_per_env or int(rows_per_env) < 1:
            raise ValueError("assign(): rows_per_env must be a positive int (the rows of one env: its agents)")
        if isinstance(member_of_env, torch.Tensor):
            t = member_of_env
            if t.device.type != "cpu":
                if t.dtype != torch.int32 or t.dim() != 1 or t.numel() < 1 or not t.is_contiguous() or t.device != self.device:
                    raise ValueError("assign(): a device table must be a contiguous int32 tensor [E] on %s" % (self.device,))
                table = t
            else:
                member_of_env = t.numpy()
                table = None
        else:
            table = None
        if table is None:
            a = np.asarray(member_of_env)
            if a.ndim != 1 or a.size < 1 or a.dtype.kind not in "iu":
                raise ValueError("assign(): member_of_env must be an int array [E] (or an int32 cuda tensor, or None)")
            if a.min() < -1 or a.max() >= self.members:
                raise ValueError("assign(): entries must lie in [-1, %d) (-1: an env nobody serves); got [%d, %d]"
                                 % (self.members, int(a.min()), int(a.max())))
        E = int(a.size if table is None else table.numel())
        if n_env is not None and E != int(n_env):
            raise ValueError("assign(): the table has %d entries, n_env is %d" % (E, int(n_env)))
        if E * int(rows_per_env) >= 2 ** 31:
            raise ValueError("assign(): E * rows_per_env = %d * %d reaches 2^31 rows" % (E, int(rows_per_env)))
        if table is None:
            table = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)
        self._enqueue_route(table, int(rows_per_env))
        self._route = (table, int(rows_per_env))

    def routing(self):
        """(counts [M], unserved, env_order) of the assignment in force, as the routing kernel built them
        (swarm_policy_bank_route_read; waits for torch's current stream): envs per member, the number of envs nobody
        serves, and the served envs in the order the kernel serves them -- by member, ascending env inside a member (numpy's
        stable argsort of the table over the served envs).  None without an assignment."""
        if self._route is None:
            return None
        E = self._route[0].numel()
        counts, order, unserved = np.zeros(self.members, np.int32), np.zeros(E, np.int32), self._ctypes.c_int32(0)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self.lib.swarm_policy_bank_route_read(self.handle, counts.ctypes.data, self._ctypes.addressof(unserved), order.ctypes.data,
                                                   self._ctypes.c_void_p(stream))
        if rc != E:
            raise RuntimeError("swarm_policy_bank_route_read returned %d: %s" % (rc, self.lib.swarm_policy_last_error().decode()))
        return counts, int(unserved.value), order[:E - int(unserved.value)]

    def sync(self, member=None):
        """FusedPolicy.sync() for member `member` (its module's current device parameters into its slice of the handle; the
        other members' bytes stay), or for all members when None: one packing launch each on torch's current stream.  Enqueue
        only; everything is validated for all the members asked for before the first launch."""
        ct = self._ctypes
        if member is None:
            which = range(self.members)
        else:
            if not 0 <= int(member) < self.members:
                raise ValueError("sync(): member %d outside [0, %d)" % (int(member), self.members))
            which = [int(member)]
        want = [(self.hidden, self.in_dim), (self.hidden,), (self.hidden, self.hidden), (self.hidden,),
                (self.hidden, self.hidden), (self.hidden,), (self.act_dim, self.hidden), (self.act_dim,)]
        for k in which:
            ps = _fc_params(self.modules[k])
            if any(tuple(t.shape) != w for t, w in zip(ps, want)):
                raise ValueError("sync(): module %d's (in_dim, hidden, act_dim) are not the handle's (%d, %d, %d); refresh() builds "
                                 "a handle for new shapes" % (k, self.in_dim, self.hidden, self.act_dim))
            if any(t.device != self.device for t in ps):
                raise ValueError("sync() reads the parameters on %s; refresh() loads parameters kept on another device" % (self.device,))
        stream = torch.cuda.current_stream(self.device).cuda_stream
        for k in which:
            ws = [t.detach() if t.dtype == torch.float32 and t.is_contiguous() else t.detach().to(torch.float32).contiguous()
                  for t in _fc_params(self.modules[k])]
            rc = self.lib.swarm_policy_bank_load_device(self.handle, k, *[ct.c_void_p(w.data_ptr()) for w in ws], ct.c_void_p(stream))
            if rc != 0:
                raise RuntimeError("swarm_policy_bank_load_device failed: " + self.lib.swarm_policy_last_error().decode())

    def __call__(self, obs, out=None, noise_scale=0.0, seed=0, step=0, log_pi=None, row_offset=0):
        """FusedPolicy.__call__ over rows that are a multiple of the members: rows [m R, (m + 1) R) by member m.  Under an
        assignment (`assign`): over its E * rows_per_env rows, the rows of env e by member member_of_env[e] (the library refuses
        another row count)."""
        if (self._route is None and isinstance(obs, torch.Tensor) and obs.shape[-1] == self.in_dim
                and (obs.numel() // self.in_dim) % self.members != 0):
            raise ValueError("FusedPolicyBank: rows %d is no multiple of the %d members" % (obs.numel() // self.in_dim, self.members))
        return super().__call__(obs, out=out, noise_scale=noise_scale, seed=seed, step=step, log_pi=log_pi, row_offset=row_offset)

    def member_of_env(self, E):
        """[E] int64: the member env e acts with.  Under an assignment (`assign`): what the routing kernel READ, rebuilt from
        `routing()` (it waits for torch's current stream) -- not the table tensor, which its owner may have rewritten since;
        -1: nobody.  Otherwise e // (E / M)."""
        E = int(E)
        if self._route is not None:
            if self._route[0].numel() != E:
                raise ValueError("member_of_env: the assignment in force is for %d envs, not %d" % (self._route[0].numel(), E))
            counts, _, order = self.routing()
            a = np.full(E, -1, np.int64)
            a[order] = np.repeat(np.arange(self.members, dtype=np.int64), counts)
            return a
        if E < 1 or E % self.members != 0:
            raise ValueError("member_of_env: E = %d is no positive multiple of the %d members" % (E, self.members))
        return np.arange(E, dtype=np.int64) // (E // self.members)


class DeviceReplay:
    """Ring buffer of per-agent transitions on the device (buffer_agent.py:40-128 semantics: rows are appended in
    blocks of one env step = E*N rows; a block that would overflow the end is written flush with the end)."""

    def __init__(self, capacity_rows, obs_dim, act_dim, device, obs_dtype=torch.float32):
        self.capacity = int(capacity_rows)
        z = lambda d, dt=torch.float32: torch.zeros((self.capacity, d), dtype=dt, device=device)
        self.obs, self.next_obs = z(obs_dim, obs_dtype), z(obs_dim, obs_dtype)
        self.act, self.act_prior = z(act_dim), z(act_dim)
        self.rew, self.done = z(1), z(1)
        self.filled_i = 0
        self.curr_i = 0

    def __len__(self):
        return self.filled_i

    def push(self, obs, act, rew, next_obs, done, act_prior=None):
        """obs/next_obs [E,N,D], act/act_prior [E,N,2], rew/done [E,N]."""
        n = obs.shape[0] * obs.shape[1]
        if n > self.capacity:
            raise ValueError("one env step (%d rows) does not fit in the replay buffer (%d rows)" % (n, self.capacity))
        if self.curr_i + n > self.capacity:                       # buffer_agent.py:97-100
            self.curr_i = self.capacity - n
        s = slice(self.curr_i, self.curr_i + n)
        self.obs[s] = obs.reshape(n, -1); self.next_obs[s] = next_obs.reshape(n, -1)
        self.act[s] = act.reshape(n, -1)
        self.rew[s] = rew.reshape(n, 1); self.done[s] = done.reshape(n, 1).to(self.done.dtype)
        if act_prior is not None:
            self.act_prior[s] = act_prior.reshape(n, -1)
        self.curr_i += n
        if self.filled_i < self.capacity:                         # buffer_agent.py:122-123: the count may overshoot the
            self.filled_i += n                                    # capacity by up to one block, exactly like the reference's
        if self.curr_i == self.capacity:
            self.curr_i = 0

    def sample(self, batch, generator=None):
        """Uniform with replacement over the rows written so far.  NOT the reference's rule (see sample_reference): that
        one ignores how much of the buffer is filled and hands out never-written zero rows early in training."""
        idx = torch.randint(0, min(self.filled_i, self.capacity), (batch,), device=self.obs.device, generator=generator)
        return self.obs[idx], self.act[idx], self.rew[idx], self.next_obs[idx], self.done[idx], self.act_prior[idx]

    def sample_reference(self, batch, generator=None, begin_index_range=300000):
        """buffer_agent.py:145-154 as is: `batch` DISTINCT rows from the window
        [begin, capacity - begin_index_range + begin), begin ~ U{0 .. begin_index_range - 1} -- a sliding window over the
        whole allocation, whatever has been written.  Needs capacity > begin_index_range + batch (the reference allocates
        2e4 steps x n_agents rows, train_assembly.py:66-69)."""
        R = int(begin_index_range)
        width = self.capacity - R
        if width < batch:
            raise ValueError("sample_reference: capacity %d leaves a window of %d rows for a batch of %d" % (self.capacity, width, batch))
        dev = self.obs.device
        begin = int(torch.randint(0, R, (1,), generator=generator, device=dev).item())
        idx = torch.randperm(width, device=dev, generator=generator)[:batch] + begin
        return self.obs[idx], self.act[idx], self.rew[idx], self.next_obs[idx], self.done[idx], self.act_prior[idx]


class ChainedReplay:
    """Replay of whole env steps in which consecutive transitions SHARE their observation rows: a ring of S = K + 1 step
    slots; transition j is (obs slot j, act/rew/done/prior of slot j, next_obs = obs slot j + 1).  A push therefore copies
    one observation block instead of two (the observations are ~97 % of a transition's bytes).  The K most recent steps
    are valid; the slot after the newest holds that step's next_obs and is excluded from sampling.  Same transitions as
    DeviceReplay / the reference's buffer (buffer_agent.py:67-128), different storage.  Call `break_chain()` when the
    next pushed obs is NOT the previous next_obs (after an env reset).

    Episode boundaries without loss: `new_chain()` SEALS the ring instead -- the slot that holds the last next_obs of the
    previous chain is kept, marked as no transition start (sample() and len() skip it), and the new chain starts in the
    slot after it (rollout_device does this on every reset).  A ring that was never sealed samples exactly as before.

    log_pi=True adds a [S, n, 1] float32 column: the log-probability of each transition's exploring action (the
    log_pi_orig of buffer_agent.py's push, what AIRL's discriminator subtracts), returned by sample(is_log_pi=True)."""

    def __init__(self, n_steps, rows_per_step, obs_dim, act_dim, device, obs_dtype=torch.float32, log_pi=False):
        self.K, self.S, self.n = int(n_steps), int(n_steps) + 1, int(rows_per_step)
        z = lambda d, dt=torch.float32: torch.zeros((self.S, self.n, d), dtype=dt, device=device)
        self.obs = z(obs_dim, obs_dtype)
        # act_prior in the env's output dtype and done as the env's uint8, so that a step can write them in place
        self.act, self.act_prior = z(act_dim), z(act_dim, obs_dtype)
        self.rew, self.done = z(1), z(1, torch.uint8)
        self.log_pi = z(1) if log_pi else None
        self.cur, self.count, self._chained = 0, 0, False
        self._sealed = set()        # slots that hold a chain's last next_obs but start no transition (new_chain)

    # zero-copy use (rollout's fused path): the policy writes its action and the env step its outputs straight into the slots
    def begin_step(self, obs):
        """Slots of the transition about to be taken: dict(obs_in = observation rows of the current slot (copied from
        `obs` unless the chain already holds them), act, rew, done, prior, next_obs, log_pi (None without the column)).
        Follow with end_step()."""
        c, nx = self.cur, (self.cur + 1) % self.S
        if not self._chained:
            self.obs[c].copy_(obs.reshape(self.n, -1))
        return dict(obs_in=self.obs[c], act=self.act[c], rew=self.rew[c], done=self.done[c], prior=self.act_prior[c],
                    next_obs=self.obs[nx], log_pi=self.log_pi[c] if self.log_pi is not None else None)

    def end_step(self):
        self._sealed.discard(self.cur)
        self.cur, self.count, self._chained = (self.cur + 1) % self.S, min(self.count + 1, self.K), True

    def __len__(self):
        return (len(self._valid_starts()) if self._sealed else self.count) * self.n

    def break_chain(self):
        """The next begin_step / push copies its obs into slot `cur` instead of assuming the chain holds it.  Hazard: slot
        `cur` is also the next_obs of the newest stored transition, and that transition stays sampleable -- after an env
        reset it is paired with the new episode's first observation.  new_chain() keeps it intact."""
        self._chained = False

    def new_chain(self, obs=None):
        """Start a new chain (an episode boundary) without corrupting the stored ones.  If slot `cur` holds the next_obs of
        the newest stored transition, that slot is sealed -- kept, marked as no transition start -- and `cur` advances by
        one (the ring's oldest step is dropped when it is full).  The new chain's first observation goes into the slot
        `cur` then points at: copied from `obs` [E,N,D] if given, else left to the caller (e.g. an env reset writing into
        self.obs[self.cur]).  Returns that slot index."""
        if self.count > 0 and (self.cur - 1) % self.S not in self._sealed:
            self._sealed.add(self.cur)
            self.cur, self.count = (self.cur + 1) % self.S, min(self.count + 1, self.K)
        if obs is not None:
            self.obs[self.cur].copy_(obs.reshape(self.n, -1))
        self._chained = True
        return self.cur

    def _advance(self, steps):
        """Bookkeeping of `steps` transitions written from slot `cur` on (rollout_device)."""
        for t in range(min(steps, self.S)):
            self._sealed.discard((self.cur + t) % self.S)
        self.cur, self.count, self._chained = (self.cur + steps) % self.S, min(self.count + steps, self.K), True

    def _valid_starts(self):
        """Slots of the stored transitions, newest first."""
        w = [(self.cur - 1 - b) % self.S for b in range(self.count)]
        return [j for j in w if j not in self._sealed]

    def push(self, obs, act, rew, next_obs, done, act_prior=None, log_pi=None):
        """log_pi [E,N] / [E,N,1] (or any shape of n elements): stored in the log-pi column (the ring must have one)."""
        n = self.n
        if obs.shape[0] * obs.shape[1] != n:
            raise ValueError("ChainedReplay takes whole env steps of %d rows" % n)
        if log_pi is not None and (self.log_pi is None or log_pi.numel() != n):
            raise ValueError("push(log_pi=): the ring needs log_pi=True and %d values per step" % n)
        c, nx = self.cur, (self.cur + 1) % self.S
        self._sealed.discard(c)
        if not self._chained:
            self.obs[c] = obs.reshape(n, -1)
        self.obs[nx] = next_obs.reshape(n, -1)
        self.act[c] = act.reshape(n, -1)
        self.rew[c] = rew.reshape(n, 1); self.done[c] = done.reshape(n, 1).to(self.done.dtype)
        if act_prior is not None:
            self.act_prior[c] = act_prior.reshape(n, -1).to(self.act_prior.dtype)
        if log_pi is not None:
            self.log_pi[c] = log_pi.reshape(n, 1)
        self.cur, self.count, self._chained = nx, min(self.count + 1, self.K), True

    def sample(self, batch, generator=None, is_log_pi=False):
        """(obs, act, rew, next_obs, done, act_prior) of `batch` uniform transitions; is_log_pi=True appends their log-pi
        [batch, 1] float32 -- the 7-tuple of buffer_agent.py's sample(..., is_log_pi=True)."""
        if is_log_pi and self.log_pi is None:
            raise ValueError("sample(is_log_pi=True) needs a ChainedReplay built with log_pi=True")
        dev = self.obs.device
        valid = self._valid_starts() if self._sealed else None
        if valid is None or len(valid) == self.count:
            back = torch.randint(0, self.count, (batch,), device=dev, generator=generator)
            j = (self.cur - 1 - back) % self.S
        else:                                   # sealed slots in the window: uniform over the transition starts only
            if not valid:
                raise ValueError("ChainedReplay.sample: no stored transition")
            pick = torch.randint(0, len(valid), (batch,), device=dev, generator=generator)
            j = torch.tensor(valid, device=dev)[pick]
        r = torch.randint(0, self.n, (batch,), device=dev, generator=generator)
        jn = (j + 1) % self.S
        out = (self.obs[j, r], self.act[j, r], self.rew[j, r], self.obs[jn, r], self.done[j, r].to(torch.float32),
               self.act_prior[j, r].to(torch.float32))
        return out + (self.log_pi[j, r],) if is_log_pi else out


# log-pi of a uniform action on [-1, 1]^2 (agents.py:91: -act_dim * log(2)) in fp32: what a coin step records
LOG_PI_UNIFORM = float(np.float32(-2.0 * np.log(2.0)))


def gaussian_log_pi(z, noise_scale):
    """GaussianNoise.log_prob (utils/noise.py) of the noise noise_scale * z, as include/swarm_policy.h states it for the fused
    kernel: z [rows, act_dim] float32 normals -> [rows] float32 -(0.5 * sum_k z_k^2) - c, the sum in k order, c the fp32
    rounding of act_dim * log(fp32(noise_scale) * sqrt(2 pi)) evaluated in double; noise_scale <= 0: -0.0."""
    import math
    rows, act_dim = z.shape
    if not noise_scale > 0:
        return torch.full((rows,), -0.0, dtype=torch.float32, device=z.device)
    c = float(np.float32(act_dim * math.log(float(np.float32(noise_scale)) * math.sqrt(2.0 * math.pi))))
    z = z.float()
    s = z[:, 0] * z[:, 0]
    for k in range(1, act_dim):
        s = s + z[:, k] * z[:, k]
    return -(0.5 * s) - c


COINS = ("batch", "env")


def explore_log_c(sigma, act_dim=2):
    """The log-pi constants of per-env noise scales, as include/swarm_policy.h states them for the scalar path: for every
    fp32 sigma[e] > 0 the fp32 rounding of act_dim * log(sigma[e] * sqrt(2 pi)) evaluated in double with libm; 0 where
    sigma[e] <= 0 or NaN (such an env records -0.0 and never reads its constant).  sigma: array-like -> float32 array."""
    import math
    s = np.asarray(sigma, dtype=np.float32).reshape(-1)
    return np.array([np.float32(act_dim * math.log(float(v) * math.sqrt(2.0 * math.pi))) if v > 0 else np.float32(0.0) for v in s],
                    dtype=np.float32)


class _Explore:
    """The per-env exploration arrays of one coin="env" call, checked and on the device: epsilon (None = 0 everywhere), sigma,
    log_c (None without log_pi), coin_out (None = not recorded).  Built before anything is enqueued."""

    def __init__(self, who, E, steps, device, epsilon, noise_scale, log_pi, log_c, coin_out):
        def vector(x, name):
            """float / array-like [E] / float32 tensor [E] on the device -> (array or tensor [E], is it the caller's tensor)"""
            if isinstance(x, torch.Tensor) and (x.is_cuda or x.device == device):
                if x.dtype != torch.float32 or tuple(x.shape) != (E,) or not x.is_contiguous() or x.device != device:
                    raise ValueError(f"{who}: a device {name} must be a contiguous float32 tensor [{E}] on {device}")
                return x, True
            a = np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float32)
            if a.ndim == 0:
                a = np.full(E, a, np.float32)
            if a.shape != (E,):
                raise ValueError(f"{who}: {name} must be a float or hold one value per env, [{E}]; got shape {a.shape}")
            return np.ascontiguousarray(a), False

        eps, eps_dev = (None, False) if (not isinstance(epsilon, torch.Tensor) and np.ndim(epsilon) == 0 and not epsilon > 0) \
            else vector(epsilon, "epsilon")
        sig, sig_dev = vector(noise_scale, "noise_scale")
        lc = None
        if log_pi:
            if log_c is not None:
                lc, lc_dev = vector(log_c, "log_c")
            elif sig_dev:
                raise ValueError(f"{who}: a cuda-tensor noise_scale with log_pi=True needs log_c= (its constants are formed on "
                                 "the host in double, rollout.explore_log_c; a device log is not pinned to that)")
            else:
                lc = explore_log_c(sig)
        elif log_c is not None:
            raise ValueError(f"{who}: log_c= is the log-pi constant; it needs log_pi=True")
        if coin_out is not None and (not isinstance(coin_out, torch.Tensor) or coin_out.dtype != torch.uint8 or coin_out.device != device
                                     or tuple(coin_out.shape) != (steps, E) or not coin_out.is_contiguous()):
            raise ValueError(f"{who}: coin_out must be a contiguous uint8 tensor [{steps}, {E}] on {device}")
        up = lambda a: a if a is None or isinstance(a, torch.Tensor) else torch.from_numpy(a).to(device)
        self.epsilon, self.sigma, self.log_c, self.coin_out, self.E = up(eps), up(sig), up(lc), coin_out, E

    def struct(self, step=0):
        """swarm_explore_t with the coins of step `step` on (a stretch of a call starts there)."""
        from . import _lib
        ptr = lambda t: t.data_ptr() if t is not None else None
        coin = self.coin_out.data_ptr() + step * self.E if self.coin_out is not None else None
        return _lib.SwarmExplore(ptr(self.epsilon), ptr(self.sigma), ptr(self.log_c), coin)


def _check_coin(who, coin, log_c, coin_out):
    if coin not in COINS:
        raise ValueError(f"{who}: coin must be 'batch' (one host coin per step for the whole batch) or 'env' (one device coin "
                         "per env and step)")
    if coin == "batch" and (log_c is not None or coin_out is not None):
        raise ValueError(f"{who}: log_c= and coin_out= belong to coin='env'")


@torch.no_grad()
def rollout(env, policy, steps, obs, replay=None, noise_scale=0.0, epsilon=0.0, generator=None, host_rng=None,
            track_reward=True, seed=0, step0=0, log_pi=False, coin="batch", log_c=None, coin_out=None):
    """Run `steps` env steps entirely on the device.

    env   : object with step_tensor(action[E,N,2]) -> (obs[E,N,D], rew[E,N], done[E,N], a_prior[E,N,2]|None)
            (marl_llm_amd.env.AssemblySwarmEnv, or a SwarmBatch through `step`)
    obs   : current observation tensor [E,N,D] (from reset_tensor / the previous rollout)
    coin="batch" (default): ONE epsilon coin of agents.py:89 per step for the whole batch, drawn on the HOST (numpy, like the
    reference's np.random.rand()).  `host_rng`: anything with a .random() method -- the np.random module (default), a
    RandomState or a Generator (np.random.default_rng).
    coin="env" (the fused path only): one coin per ENV and step, as E copies of the reference's loop flip it, drawn on the
    device by a counter-based generator keyed by (seed, step0 + t, env) -- no host synchronisation and no host RNG.  epsilon
    and noise_scale may each be a float, an array-like [E] or a float32 cuda tensor [E]; log_c and coin_out ([steps, E] uint8)
    as in rollout_device.  Per step: the actor without noise, then swarm_explore_envs (include/swarm_rollout.h) in place on
    the ring slot.  This loop is the witness of rollout_device(coin="env"): the same bits.

    Fused path (policy is a FusedPolicy, replay a ChainedReplay, env a SwarmBatch): TWO launches per step and no copies --
    the policy kernel adds the exploration noise in its epilogue (counter-based generator keyed by (seed, step0 + t, row))
    and writes the action into the replay slot; the env step writes next_obs / reward / done / prior into the ring.
    Everywhere else: the policy's action + torch noise, then `replay.push`.
    track_reward: also return the mean reward of every step ([steps] tensor; one small reduction per step).
    log_pi: also store each transition's log-probability of its exploring action (agents.py:78-96's log_pi) in the ring's
            log-pi column -- the fused kernel's (FusedPolicy), gaussian_log_pi of the torch normals (any other module), or
            LOG_PI_UNIFORM on a coin step.  Needs a ChainedReplay built with log_pi=True.
    Returns (last obs, mean reward per step tensor [steps] or None)."""
    import numpy as np
    from .batched import SwarmBatch
    if log_pi and not (isinstance(replay, ChainedReplay) and replay.log_pi is not None):
        raise ValueError("rollout(log_pi=True) needs a ChainedReplay built with log_pi=True")
    step = env.step_tensor if hasattr(env, "step_tensor") else env.step
    E, N, D = obs.shape
    rews = torch.zeros(steps, device=obs.device) if track_reward else None
    fused = isinstance(policy, FusedPolicy) and isinstance(replay, ChainedReplay) and isinstance(env, SwarmBatch)
    _check_coin("rollout", coin, log_c, coin_out)
    per_env = None
    if coin == "env":
        if not fused:
            raise ValueError("rollout(coin='env') runs on the fused path: a FusedPolicy, a ChainedReplay and a SwarmBatch")
        import ctypes
        from . import _lib
        per_env = _Explore("rollout", E, steps, policy.device, epsilon, noise_scale, log_pi, log_c, coin_out)
        m64 = 2 ** 64 - 1
    draw = host_rng if host_rng is not None else np.random
    for t in range(steps):
        explore_uniform = per_env is None and epsilon > 0 and draw.random() < epsilon                 # agents.py:89-91
        if per_env is not None:
            sl = replay.begin_step(obs)
            policy(sl["obs_in"], out=sl["act"], noise_scale=0.0, seed=seed, step=step0 + t)
            ex = per_env.struct()
            rc = policy.lib.swarm_explore_envs(sl["act"].data_ptr(), sl["log_pi"].data_ptr() if log_pi else None, E * N, N,
                                               ctypes.byref(ex), coin_out[t].data_ptr() if coin_out is not None else None,
                                               int(seed) & m64, (int(step0) + t) & m64, 0,
                                               ctypes.c_void_p(torch.cuda.current_stream(policy.device).cuda_stream))
            if rc != 0:
                raise _lib.SwarmError(f"libswarmenv error {rc}: {policy.lib.swarm_rollout_last_error().decode()}")
            next_obs, rew, done, pri = env.step(sl["act"].view(E, N, 2),
                                                out=dict(obs=sl["next_obs"], rew=sl["rew"], done=sl["done"], prior=sl["prior"]))
            replay.end_step()
        elif fused:
            sl = replay.begin_step(obs)
            if explore_uniform:
                sl["act"].copy_(torch.rand((E * N, policy.act_dim), device=obs.device, generator=generator) * 2 - 1)
                if log_pi:
                    sl["log_pi"].fill_(LOG_PI_UNIFORM)
            else:
                policy(sl["obs_in"], out=sl["act"], noise_scale=noise_scale, seed=seed, step=step0 + t,
                       log_pi=sl["log_pi"].view(-1) if log_pi else None)
            next_obs, rew, done, pri = env.step(sl["act"].view(E, N, 2),
                                                out=dict(obs=sl["next_obs"], rew=sl["rew"], done=sl["done"], prior=sl["prior"]))
            replay.end_step()
        else:
            x = obs.reshape(E * N, D)
            if x.dtype != torch.float32 and not (x.dtype == torch.bfloat16 and isinstance(policy, FusedPolicy)):
                x = x.float()
            lp = None
            if explore_uniform:
                act = torch.rand((E * N, 2), device=obs.device, generator=generator) * 2 - 1
                if log_pi:
                    lp = torch.full((E * N,), LOG_PI_UNIFORM, device=obs.device)
            elif isinstance(policy, FusedPolicy):
                act = policy(x, noise_scale=noise_scale, seed=seed, step=step0 + t, log_pi=True if log_pi else None)  # noise in the kernel's epilogue
                if log_pi:
                    act, lp = act
            else:
                act = policy(x)
                z = None
                if noise_scale > 0:                                                                    # agents.py:93-96
                    z = torch.randn(act.shape, device=obs.device, generator=generator)
                    act = (act + noise_scale * z).clamp_(-1, 1)
                if log_pi:
                    lp = gaussian_log_pi(z if z is not None else act, noise_scale)
            act = act.reshape(E, N, 2)
            next_obs, rew, done, pri = step(act)
            if replay is not None:
                if log_pi:
                    replay.push(obs, act, rew, next_obs, done, pri, log_pi=lp)
                else:
                    replay.push(obs, act, rew, next_obs, done, pri)
        if track_reward:
            rews[t] = rew.mean()
        obs = next_obs
    return obs, rews


def _is_view_of(t, slot):
    return (isinstance(t, torch.Tensor) and t.device == slot.device and t.dtype == slot.dtype and t.data_ptr() == slot.data_ptr()
            and t.numel() == slot.numel() and t.is_contiguous())


@torch.no_grad()
def rollout_device(env, policy, steps, obs=None, replay=None, noise_scale=0.0, epsilon=0.0, host_rng=None, seed=0, step0=0,
                   row_offset=0, reset=None, track_reward=True, log_pi=False, resets=None, coin="batch", log_c=None, coin_out=None):
    """`steps` exploring-actor + env steps in ONE library call (swarm_rollout, include/swarm_rollout.h): the launches are
    enqueued on torch's current stream and the call returns without a host synchronisation.

    env      : a SwarmBatch, or an AssemblySwarmEnv (agent_strategy 'input', not is_collected) through its backend.
    policy   : a FusedPolicy (noise keyed by (seed, step0 + t, row_offset + row), swarm_policy.h).
    replay   : a ChainedReplay (f32 or bf16 obs, the env's dtype), or None: a private two-slot ring kept on the env, whose
               slots the next rollout_device call on that env reuses (the returned obs then stays valid for one more call).
    obs / reset: the chain.  `obs` equal to the ring slot replay.obs[replay.cur] (what the previous call returned), or None
               with a chained ring, continues it.  Any other `obs` [E,N,D], or reset=(seed, episode[, env_offset]) -- the
               device reset swarm_reset writing straight into the ring (SwarmBatch only; the shape set must be uploaded) --
               starts a new chain through replay.new_chain(): the stored transitions keep their true next_obs.
    epsilon  : the coin of agents.py:89-91, drawn on the host before the call, one host_rng.random() per step (the order and
               count rollout() uses); a coin step takes counter-based uniform actions instead of the policy.
    coin     : "batch" (default) -- the line above: one host coin per step, every env of the batch explores uniformly at the
               same instant.  "env" -- one coin per ENV and step, what E independent copies of the reference's episode loop
               flip (swarm_rollout_explore, include/swarm_rollout.h "Per-env exploration"): drawn on the device in stream
               order from (seed, step0 + t, row_offset // N + e), so host_rng is not consumed and the call is a function of
               its arguments alone, on any rank (row_offset must be a multiple of N).  epsilon and noise_scale may then each
               be a float, an array-like [E] or a float32 cuda tensor [E] -- an exploration spectrum over the width of the
               batch; device tensors are read when the kernels run (values written on the stream before the call are seen)
               and cost no upload.  With epsilon 0 and one noise_scale the result is bit for bit coin="batch"'s.
    log_c    : coin="env" with log_pi=True: the log-pi constants [E] (explore_log_c).  Computed on the host in double from the
               fp32 noise_scale unless given; a cuda-tensor noise_scale needs it given (ValueError otherwise).
    coin_out : coin="env": a uint8 cuda tensor [steps, E] that receives 1 where env e took the uniform branch at step t.
    resets   : {step: (seed, episode[, env_offset])} with 0 <= step < steps -- episode boundaries inside the call (SwarmBatch
               only; EpisodeClock writes such schedules).  An int episode is the whole-batch reset, an int array-like /
               int64 cuda tensor [E] the per-env one (SwarmBatch.reset_envs: -1 keeps the env).  The reset of step t comes
               before everything else of step t.  It ends a chain: the slot that holds step t-1's next_obs is sealed
               (new_chain) and the reset writes its observation of all envs into the slot behind it, so every stored
               transition keeps its true next_obs and each cut costs ONE ring slot for the whole batch -- group the envs
               (EpisodeClock's groups) to keep that small.  The call is split into stretches: a reset, then one library call
               up to the next reset (noise keyed by step0 + t as ever); without entries it stays one library call.
               resets={0: (seed, ep)} is reset=(seed, ep); both together are a ValueError.  The whole schedule is checked
               and uploaded before anything is enqueued.
    log_pi   : also record each transition's log-probability of its exploring action (swarm_rollout_logpi) in the ring's
               log-pi column: the policy kernel's (include/swarm_policy.h) or LOG_PI_UNIFORM on a coin step -- what
               train_assembly_airl.py pushes as log_pi_orig.  The ring must be built with log_pi=True (the private ring
               gets the column on request); the actions and the rest of the ring are the same bits as without it.
    Returns (obs [E,N,D] -- the ring slot of the last next_obs --, reward_stats [steps, 2] float64 (mean, population std
    per step; train_assembly.py:109-110) or None).  On error nothing is enqueued, the ring is unchanged, SwarmError raises
    (ValueError for a ring without the log-pi column)."""
    import ctypes
    import numpy as np
    from . import _lib
    aenv, sb = _device_env(env, "rollout_device", lambda e: e.agent_strategy == "input" and not e.is_collected,
                           "rollout_device drives the env with the policy's actions: needs agent_strategy 'input' and not is_collected",
                           reset if reset is not None else (resets or None))
    if not isinstance(policy, FusedPolicy):
        raise TypeError("rollout_device needs a FusedPolicy (the device loop runs the fused policy kernel)")
    steps = int(steps)
    if steps < 0:
        raise ValueError("steps must be >= 0")
    plan = _reset_plan(sb, resets, steps, reset, "rollout_device")
    first = reset if reset is not None else plan.get(0)
    E, N, D = sb.n_env, sb.n_agents, sb.obs_dim
    replay = _device_ring(sb, replay, log_pi)
    if log_pi and replay.log_pi is None:
        raise ValueError("rollout_device(log_pi=True) needs a ChainedReplay built with log_pi=True")
    _check_coin("rollout_device", coin, log_c, coin_out)
    # coin="env": the arrays are checked and uploaded here, before the ring is touched and before anything is enqueued
    per_env = _Explore("rollout_device", E, steps, sb.device, epsilon, noise_scale, log_pi, log_c, coin_out) if coin == "env" else None
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream(sb.device).cuda_stream)

    def call(k, coins, stats, a=0):
        ring = _ring_struct(sb, replay)
        keys = (int(seed) & (2 ** 64 - 1), (int(step0) + a) & (2 ** 64 - 1), int(row_offset) & (2 ** 64 - 1),
                ctypes.c_void_p(stats[a:].data_ptr()) if stats is not None else None, stream)
        if per_env is not None:
            ex = per_env.struct(a)
            rc = lib.swarm_rollout_explore(sb.handle, policy.handle, ctypes.byref(ring),
                                           ctypes.c_void_p(replay.log_pi.data_ptr()) if log_pi else None, k, ctypes.byref(ex), *keys)
            return _check_rollout(lib, rc, k, first)
        tail = (k, coins.ctypes.data_as(ctypes.c_void_p) if coins is not None else None, float(noise_scale)) + keys
        if log_pi:
            rc = lib.swarm_rollout_logpi(sb.handle, policy.handle, ctypes.byref(ring), ctypes.c_void_p(replay.log_pi.data_ptr()), *tail)
        else:
            rc = lib.swarm_rollout(sb.handle, policy.handle, ctypes.byref(ring), *tail)
        _check_rollout(lib, rc, k, first)

    coins = None
    if per_env is None and epsilon > 0:
        draw = host_rng if host_rng is not None else np.random
        coins = np.array([draw.random() < epsilon for _ in range(steps)], dtype=np.uint8)          # agents.py:89
    stats = torch.empty((steps, 2), dtype=torch.float64, device=sb.device) if track_reward else None
    _run_stretches(aenv, sb, replay, obs, reset, plan, steps, lambda: call(0, None, None),
                   lambda a, b: call(b - a, np.ascontiguousarray(coins[a:b]) if coins is not None else None, stats, a), "rollout_device")
    return replay.obs[replay.cur].view(E, N, D), stats


# ---- chain handling shared by rollout_device and rollout_expert
def _device_env(env, who, strategy_ok, strategy_msg, reset):
    """(AssemblySwarmEnv or None, SwarmBatch) of a device-loop call; the env's strategy is checked before anything runs."""
    from .batched import SwarmBatch
    if isinstance(env, SwarmBatch):
        return None, env
    if hasattr(env, "_flush_cells") and hasattr(env, "agent_strategy"):
        if not strategy_ok(env):
            raise ValueError(strategy_msg)
        if reset is not None:
            raise ValueError("reset= needs a SwarmBatch; with an AssemblySwarmEnv call reset_tensor() and pass its obs")
        return env, env._flush_cells()
    raise TypeError("env must be a SwarmBatch or an AssemblySwarmEnv")


def _device_ring(sb, replay, log_pi=False):
    """The caller's ChainedReplay, or the private two-slot ring kept on the env (given a log-pi column if log_pi)."""
    if replay is None:
        replay = getattr(sb, "_rollout_ring", None)
        if replay is None:
            replay = sb._rollout_ring = ChainedReplay(1, sb.n_env * sb.n_agents, sb.obs_dim, 2, sb.device, obs_dtype=sb.obs_dtype)
        if log_pi and replay.log_pi is None:
            replay.log_pi = torch.zeros((replay.S, replay.n, 1), dtype=torch.float32, device=sb.device)
    elif not isinstance(replay, ChainedReplay):
        raise TypeError("replay must be a ChainedReplay (or None)")
    return replay


def _ring_struct(sb, replay):
    from . import _lib
    dt_code = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float64: _lib.F64}[replay.obs.dtype]
    return _lib.SwarmRing(replay.obs.data_ptr(), replay.act.data_ptr(), replay.rew.data_ptr(), replay.done.data_ptr(),
                          replay.act_prior.data_ptr() if sb.with_prior else None, replay.n, replay.obs.shape[-1], dt_code,
                          replay.S, replay.cur)


def _check_rollout(lib, rc, k, reset):
    from . import _lib
    if rc != 0 and not (k == 0 and rc == 3 and reset is not None):    # SWARM_ERR_STATE (not observed): the reset observes
        raise _lib.SwarmError(f"libswarmenv error {rc}: {lib.swarm_rollout_last_error().decode()}")


def _begin_chain(sb, replay, obs, reset, validate, who, upload=None):
    """Continue the ring's chain, or start a new one from `obs` / reset=(seed, episode[, env_offset]) through
    replay.new_chain().  `validate()` (a zero-step library call) runs first: a rejected call leaves the ring as it was.
    reset may also be a callable that returns the (uploaded) step-0 entry of a resets= schedule; upload() -- the uploads of
    that schedule -- runs behind validate() and before anything is enqueued."""
    E, N, D = sb.n_env, sb.n_agents, sb.obs_dim
    n = E * N
    cont = reset is None and (obs is None or _is_view_of(obs, replay.obs[replay.cur]))
    if cont and obs is None and not replay._chained:
        raise ValueError(f"{who}: the ring holds no current observation; pass obs or reset=")
    if not cont and obs is not None and (not isinstance(obs, torch.Tensor) or obs.device != sb.device or obs.dtype != sb.obs_dtype
                                         or obs.numel() != n * D):
        raise ValueError(f"obs must be a {sb.obs_dtype} tensor [{E}, {N}, {D}] on {sb.device}")
    validate()                              # validation only: a rejected call raises before the ring is touched
    if upload is not None:
        upload()
    if not cont:
        kept = (replay.cur, replay.count, replay._chained, set(replay._sealed))
        try:
            if reset is not None:
                _chain_reset(sb, replay, reset() if callable(reset) else reset)
            else:
                replay.new_chain(obs)
        except Exception:
            replay.cur, replay.count, replay._chained, replay._sealed = kept
            raise


def _chain_reset(sb, replay, entry):
    """An episode boundary in the ring: seal the slot that holds the last next_obs (new_chain) and let the reset -- the whole
    batch's for an int episode, the per-env one for an uploaded episode vector (SwarmBatch._episode_upload's pair) -- write
    its observation of ALL envs into the slot behind it.  A kept env's row there equals its row in the sealed slot."""
    r = tuple(entry)
    seed, episode, env_offset = r[0], r[1], r[2] if len(r) > 2 else 0
    slot = replay.new_chain()
    if isinstance(episode, tuple):
        sb._reset_envs_ready(seed, episode, env_offset, out=replay.obs[slot])
    else:
        sb.reset(seed, episode, env_offset, out=replay.obs[slot])


def _reset_plan(sb, resets, steps, reset, who):
    """resets= of the device loops, checked on the host: {step: (seed, episode, env_offset)} in step order, where episode is
    an int (a whole-batch swarm_reset) or SwarmBatch._episode_args' checked vector (reset_envs).  Raises before anything
    is uploaded or enqueued."""
    if resets is None:
        return {}
    if not isinstance(resets, dict):
        raise ValueError(f"{who}: resets= must be a dict {{step: (seed, episode[, env_offset])}}")
    plan = {}
    for t, entry in resets.items():
        if int(t) != t or not 0 <= int(t) < steps:
            raise ValueError("resets: step %r outside [0, %d)" % (t, steps))
        r = tuple(entry)
        if len(r) not in (2, 3):
            raise ValueError("resets: the entry of step %d must be (seed, episode[, env_offset])" % int(t))
        episode = r[1]
        if (isinstance(episode, torch.Tensor) and episode.dim() > 0) or (not isinstance(episode, torch.Tensor) and np.ndim(episode) > 0):
            episode = sb._episode_args(episode)
        else:
            if int(episode) != episode or int(episode) < 0:
                raise ValueError("resets: the whole-batch episode of step %d must be an int >= 0, got %r" % (int(t), episode))
            episode = int(episode)
        plan[int(t)] = (int(r[0]), episode, int(r[2]) if len(r) > 2 else 0)
    if reset is not None and 0 in plan:
        raise ValueError(f"{who}: reset= and resets[0] both reset the envs at step 0; give one")
    if plan and sb.n_shapes < 1:
        from . import _lib
        raise _lib.SwarmError(f"{who}: resets= needs a shape set (SwarmBatch.set_shapes)")
    return dict(sorted(plan.items()))


def _run_stretches(aenv, sb, replay, obs, reset, plan, steps, validate, stretch, who, splits=()):
    """The chain of one device-loop call with a resets= plan: begin the chain (obs / reset= / the plan's step 0), then for
    every stretch between two resets the reset (_chain_reset) and ONE library call, stretch(a, b), for steps [a, b) with
    the ring at replay.cur; the ring advances by the stretch and its seal.  Without a plan that is one call.  splits:
    further steps at which the caller wants a stretch to end (rollout_eval's per-env switches).  Everything is checked and
    uploaded before the first enqueue; if anything raises the ring is put back exactly as it was."""
    kept = (replay.cur, replay.count, replay._chained, set(replay._sealed))

    def upload():
        for t, (seed, episode, off) in plan.items():
            if not isinstance(episode, int):
                plan[t] = (seed, sb._episode_upload(episode), off)

    try:
        _begin_chain(sb, replay, obs, (lambda: plan[0]) if 0 in plan else reset, validate, who, upload)
        starts = sorted(set(plan) | set(splits) | {0})
        for a, b in zip(starts, starts[1:] + [steps]):
            if a > 0 and a in plan:
                _chain_reset(sb, replay, plan[a])
            stretch(a, b)
            replay._advance(b - a)
    except Exception:
        replay.cur, replay.count, replay._chained, replay._sealed = kept
        raise
    if aenv is not None:
        aenv.simulation_time += aenv.dt * steps
        aenv._state_version += 1


class EpisodeClock:
    """Staggered episodes for the device loops, host only: which env starts which episode at which global step.

    Env e belongs to group e % groups and starts q_e = (group * episode_len) // groups steps into its episode 0.  At global
    step t it resets iff t == 0 or (t + q_e) % episode_len == 0, and its episode number then is (t + q_e) // episode_len.
    resets(steps) returns the resets= dict of the next `steps` global steps and advances the clock: an int entry (the
    whole-batch reset) where every env resets with one episode number, an int64 vector (-1 = keep) elsewhere.  groups=1 is
    today's in-phase batch: int entries every episode_len steps.  Each cut costs the ring one slot for the whole batch
    (rollout_device), i.e. groups slots per episode_len steps.

        clock = EpisodeClock(E, 200, groups=8, seed=7)
        obs, stats = rollout_device(sb, pol, K, replay=ring, resets=clock.resets(K))"""

    def __init__(self, n_env, episode_len, groups=1, seed=0, env_offset=0):
        n_env, episode_len, groups = int(n_env), int(episode_len), int(groups)
        if n_env < 1 or episode_len < 1 or not 1 <= groups <= episode_len:
            raise ValueError("EpisodeClock needs n_env >= 1, episode_len >= 1 and 1 <= groups <= episode_len")
        self.n_env, self.episode_len, self.groups = n_env, episode_len, groups
        self.seed, self.env_offset = int(seed), int(env_offset)
        self.t = 0

    def resets(self, steps):
        steps, L, t0 = int(steps), self.episode_len, self.t
        groups = min(self.groups, self.n_env)                  # the groups that hold an env
        due = {}                                               # global step -> {group: episode}; the work is per group, not per step
        for g in range(groups):
            q = (g * L) // self.groups
            t = t0 + (-(t0 + q)) % L                           # the first t >= t0 with (t + q) % L == 0
            while t < t0 + steps:
                due.setdefault(t, {})[g] = (t + q) // L
                t += L
        if t0 == 0 and steps > 0:
            due[0] = {g: 0 for g in range(groups)}             # every env starts its episode 0 at t = 0
        out = {}
        for t in sorted(due):
            episode = due[t]
            if len(episode) == groups and len(set(episode.values())) == 1:
                out[t - t0] = (self.seed, episode[0], self.env_offset)
            else:
                by_group = np.full(self.groups, -1, np.int64)
                by_group[list(episode)] = list(episode.values())
                out[t - t0] = (self.seed, by_group[np.arange(self.n_env) % self.groups], self.env_offset)
        self.t += steps
        return out


@torch.no_grad()
def rollout_expert(env, steps, obs=None, replay=None, reset=None, source="rule", track_reward=True, resets=None):
    """`steps` expert steps in ONE library call (swarm_rollout_expert, include/swarm_rollout.h): the device counterpart of
    collect_expert_data.py's loop (agent_strategy 'rule' / 'llm' with is_collected).  Enqueued on torch's current stream;
    returns without a host synchronisation.

    env    : a SwarmBatch, or an AssemblySwarmEnv whose agent_strategy is `source` (its float32 / bfloat16 backend).  Up to
             256 agents on a default batch, 257 to 1024 on a large_swarm one (both sources).
    source : "rule" -- the rule-based expert (assembly.py:530-601) computed on the device in fp64 (bit-identical to
             SwarmBatch.rule_action()); the env steps with that fp64 action and the ring's act row holds its f32 rounding.
             "llm"  -- the prior policy's twin (a batch created with llm_action): the ring's act row is the applied action,
             what the eager path returns as its fifth value with is_collected.
    replay / obs / reset / resets : the chain, exactly as rollout_device (reset= seals the boundary slot through new_chain();
             resets= puts whole-batch and per-env episode boundaries inside the call, one library call per stretch).
    Returns (obs [E,N,D] -- the ring slot of the last next_obs --, reward_stats [steps, 2] float64 or None).  On error
    nothing is enqueued, the ring and the env state are unchanged, and SwarmError / ValueError raises."""
    import ctypes
    from . import _lib
    if source not in ("rule", "llm"):
        raise ValueError("source must be 'rule' or 'llm'")
    aenv, sb = _device_env(env, "rollout_expert", lambda e: e.agent_strategy == source,
                           f"rollout_expert(source={source!r}) needs an AssemblySwarmEnv with agent_strategy {source!r}",
                           reset if reset is not None else (resets or None))
    steps = int(steps)
    if steps < 0:
        raise ValueError("steps must be >= 0")
    plan = _reset_plan(sb, resets, steps, reset, "rollout_expert")
    first = reset if reset is not None else plan.get(0)
    E, N, D = sb.n_env, sb.n_agents, sb.obs_dim
    replay = _device_ring(sb, replay)
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream(sb.device).cuda_stream)
    src = _lib.EXPERT_RULE if source == "rule" else _lib.EXPERT_LLM

    def call(k, stats, a=0):
        ring = _ring_struct(sb, replay)
        rc = lib.swarm_rollout_expert(sb.handle, ctypes.byref(ring), k, src,
                                      ctypes.c_void_p(stats[a:].data_ptr()) if stats is not None else None, stream)
        _check_rollout(lib, rc, k, first)

    stats = torch.empty((steps, 2), dtype=torch.float64, device=sb.device) if track_reward else None
    _run_stretches(aenv, sb, replay, obs, reset, plan, steps, lambda: call(0, None), lambda a, b: call(b - a, stats, a), "rollout_expert")
    return replay.obs[replay.cur].view(E, N, D), stats


EXPERT_KEYS = ("obs_buffs", "ac_buffs", "next_obs_buffs", "done_buffs")       # ReplayBufferExpert.save (buffer_expert.py)


@torch.no_grad()
def save_expert_data(replay, file_dir, dtype=np.float64):
    """Write `file_dir`/expert_data.npz from a ChainedReplay, with exactly ReplayBufferExpert.save's keys: obs_buffs [L, D],
    ac_buffs [L, 2], next_obs_buffs [L, D], done_buffs [L, 1], all in `dtype`.  ReplayBufferExpert.load reads it unchanged.

    Rows are the ring's stored transitions, oldest step first; within a step env-major, then agent -- the order
    ReplayBufferExpert.push produces from the numpy API, whose agent axis holds the envs side by side.  Sealed slots (the
    last next_obs of a chain, see ChainedReplay.new_chain) start no transition and are skipped, so no row pairs one
    episode's last observation with the next episode's first.

    Differences from the reference's file: it holds only written rows (the reference saves its whole allocation, zero rows
    included, once it is not yet full), and in chronological order (the reference's in ring order after a wrap-around).
    train_assembly_airl.py sets total_length from the loaded shape, so it works unchanged.  The data streams to the file
    one ring slot at a time (no host or device copy of the whole ring).  Returns the file's path."""
    import os
    import zipfile
    starts = replay._valid_starts()[::-1]                           # oldest first
    n, S, D = replay.n, replay.S, replay.obs.shape[-1]
    L = len(starts) * n
    dt = np.dtype(dtype)
    src = {"obs_buffs": (lambda j: replay.obs[j], D), "ac_buffs": (lambda j: replay.act[j], 2),
           "next_obs_buffs": (lambda j: replay.obs[(j + 1) % S], D), "done_buffs": (lambda j: replay.done[j], 1)}
    os.makedirs(file_dir, exist_ok=True)
    path = os.path.join(file_dir, "expert_data.npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_STORED, allowZip64=True) as zf:    # np.savez's container
        for key in EXPERT_KEYS:
            rows, width = src[key]
            with zf.open(key + ".npy", "w", force_zip64=True) as f:
                np.lib.format.write_array_header_1_0(f, {"descr": np.lib.format.dtype_to_descr(dt), "fortran_order": False,
                                                         "shape": (L, width)})
                for j in starts:
                    t = rows(j)
                    if t.dtype == torch.bfloat16:
                        t = t.float()                               # exact; numpy has no bfloat16
                    f.write(np.ascontiguousarray(t.reshape(n, width).cpu().numpy().astype(dt, copy=False)).data)
    return path


# ---- evaluation (eval_assembly.py:119-205)
METRIC_KEYS = ("coverage_rate", "uniformity_degree", "voronoi_uniformity")     # eval_assembly.py:168-174, trace.metrics[..., k]


class EvalTrace:
    """What rollout_eval recorded: metrics [steps, E, 3] float64 (coverage_rate, distribution_uniformity,
    voronoi_based_uniformity of the state BEFORE step t against the cells in force at step t), p / dp [steps, E, 2, N]
    float64 (that state) or None, reward_stats [steps, 2] float64 or None -- device tensors, valid once the stream has run --
    and shape [steps], a host int array: the shape index every env was switched to and that is in force at step t, or -1
    while no switch has happened (cells set by hand, or drawn per env by a reset) and at steps where the envs differ (per-env
    switches).  shape_env [steps, E], a host int array: the shape env e was switched to and holds at step t, -1 where that is
    not known; None if a per-env entry's index was a device tensor."""

    def __init__(self, metrics, p=None, dp=None, reward_stats=None, shape=None, shape_env=None):
        self.metrics, self.p, self.dp, self.reward_stats = metrics, p, dp, reward_stats
        self.shape = np.full(len(metrics), -1, np.int64) if shape is None else np.asarray(shape, dtype=np.int64)
        self.shape_env = None if shape_env is None else np.asarray(shape_env, dtype=np.int64)


def _per_env_entry(sh):
    """An entry of switch= that names a shape per env: a dict of select_shapes' arguments, or an array-like / tensor [E]."""
    return isinstance(sh, dict) or (sh is not None and (isinstance(sh, torch.Tensor) and sh.dim() > 0 or
                                                        not isinstance(sh, torch.Tensor) and np.ndim(sh) > 0))


def _switch_schedule(switch, steps, per_env=None):
    """switch= of rollout_eval as the int32 [steps] array swarm_rollout_eval takes (-1 = keep), or None without a batch-wide
    switch: a {step: shape_index} dict, or a sequence of length `steps` (-1 / None = keep).  per_env: a dict that receives
    the per-env entries as {step: dict of select_shapes' arguments} (an array entry becomes {"index": array}); without it
    such an entry is a ValueError."""
    if switch is None:
        return None
    sched = np.full(steps, -1, np.int32)

    def entry(t, sh, keep_ok):
        if _per_env_entry(sh):
            if per_env is None:
                raise ValueError("switch: a per-env entry at step %d where only shape indices are taken" % t)
            kw = dict(sh) if isinstance(sh, dict) else {"index": sh}
            if "index" not in kw or set(kw) - {"index", "angle", "offset", "pose"}:
                raise ValueError("switch: a per-env entry takes index and angle / offset / pose, got %r" % sorted(kw))
            per_env[t] = kw
        else:
            sched[t] = _shape_entry(sh, keep_ok)

    if isinstance(switch, dict):
        for t, sh in switch.items():
            if int(t) != t or not 0 <= int(t) < steps:
                raise ValueError("switch: step %r outside [0, %d)" % (t, steps))
            entry(int(t), sh, False)
    else:
        seq = list(switch)
        if len(seq) != steps:
            raise ValueError("switch: a sequence must have one entry per step (%d), got %d" % (steps, len(seq)))
        for t, sh in enumerate(seq):
            if sh is not None:
                entry(t, sh, True)
    return sched if (sched >= 0).any() else None


def _shape_entry(sh, keep_ok=False):
    if int(sh) != sh or int(sh) < (-1 if keep_ok else 0) or int(sh) >= 2 ** 31:
        raise ValueError("switch: shape index %r is not a valid index" % (sh,))
    return int(sh)


@torch.no_grad()
def rollout_eval(env, policy, steps, obs=None, replay=None, reset=None, switch=None, trace_state=False, track_reward=True,
                 resets=None):
    """`steps` evaluation steps in ONE library call (swarm_rollout_eval, include/swarm_rollout.h): the device counterpart of
    eval_assembly.py:145-186 for every env of the batch.  Per step: the state trace, an optional target-shape switch on the
    device, the three wrapper metrics, the actor WITHOUT noise (explore=False) at the policy's precision, the env step.
    Enqueued on torch's current stream; returns without waiting for the GPU.

    env / policy / replay / obs / reset : exactly as rollout_device (the ring records the evaluation transitions; the
             private two-slot ring is enough for evaluation).
    switch : {step: entry} or a sequence of length `steps` (-1 / None = keep).  An int entry: at that step every env takes
             that shape of the uploaded set (SwarmBatch.set_shapes) at the set's own pose, before the step's metrics --
             process_shape of eval_assembly.py:34-57.  A per-env entry -- an int array-like / tensor [E], or a dict with
             select_shapes' keys (index, angle, offset, pose) -- gives every env its own shape and pose, or lets it keep what
             it has (SwarmBatch.select_shapes).  The actor at a switch step still sees the observation the previous step
             returned (computed against the old shape), as the reference's does.  A schedule of ints is one library call; one
             with per-env entries is split at those steps -- select_shapes, then swarm_rollout_eval for the stretch up to the
             next -- with the same results as the eager loop, bit for bit.  Every host array of the schedule is checked and
             uploaded before the first stretch is enqueued.  Needs a SwarmBatch; ValueError with an AssemblySwarmEnv (assign
             its grid_center / n_g / l_cell between calls instead).
    resets : episode boundaries inside the call, as rollout_device's resets= (SwarmBatch only).  The reset of step t comes
             before the state trace, the switch and the metrics of step t: p[t] is the fresh state, metrics[t] what metrics()
             gives behind the reset.  The call is split at those steps as it is at per-env switches.
    trace_state : also record p / dp before every step.
    Returns (obs [E,N,D] -- the ring slot of the last next_obs --, EvalTrace).  On error nothing is enqueued, the ring and
    the env are unchanged, and SwarmError / ValueError raises."""
    import ctypes
    from . import _lib
    if switch is not None and not hasattr(env, "select_shape"):
        if hasattr(env, "_flush_cells"):
            raise ValueError("switch= needs a SwarmBatch with a shape set; an AssemblySwarmEnv switches through its grid_center / "
                             "n_g / l_cell attributes between calls")
    aenv, sb = _device_env(env, "rollout_eval", lambda e: e.agent_strategy == "input" and not e.is_collected,
                           "rollout_eval drives the env with the policy's actions: needs agent_strategy 'input' and not is_collected",
                           reset if reset is not None else (resets or None))
    if not isinstance(policy, FusedPolicy):
        raise TypeError("rollout_eval needs a FusedPolicy (the device loop runs the fused policy kernel)")
    steps = int(steps)
    if steps < 0:
        raise ValueError("steps must be >= 0")
    plan = _reset_plan(sb, resets, steps, reset, "rollout_eval")
    first = reset if reset is not None else plan.get(0)
    per_env = {}
    sched = _switch_schedule(switch, steps, per_env)
    if sched is not None or per_env:
        if sb.n_shapes < 1:
            raise _lib.SwarmError("rollout_eval: switch= needs a shape set (SwarmBatch.set_shapes)")
        if sched is not None and int(sched.max()) >= sb.n_shapes:
            raise ValueError("switch: shape index %d outside [0, %d)" % (int(sched.max()), sb.n_shapes))
    checked = {t: sb._shapes_args(**kw) for t, kw in sorted(per_env.items())}     # every entry, before any upload
    E, N, D = sb.n_env, sb.n_agents, sb.obs_dim
    replay = _device_ring(sb, replay)
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream(sb.device).cuda_stream)

    def call(k, sw, out):
        ring = _ring_struct(sb, replay)                   # (the ring advances with every stretch: _run_stretches)
        rc = lib.swarm_rollout_eval(sb.handle, policy.handle, ctypes.byref(ring), k,
                                    sw.ctypes.data_as(ctypes.c_void_p) if sw is not None else None,
                                    ctypes.byref(out) if out is not None else None, stream)
        _check_rollout(lib, rc, k, first)

    ready = {}
    f64 = dict(dtype=torch.float64, device=sb.device)
    metrics = torch.empty((steps, E, 3), **f64)
    p = torch.empty((steps, E, 2, N), **f64) if trace_state else None
    dp = torch.empty((steps, E, 2, N), **f64) if trace_state else None
    stats = torch.empty((steps, 2), **f64) if track_reward else None
    ptr = lambda t, a: t[a:].data_ptr() if t is not None else None
    shape, shape_env = np.full(steps, -1, np.int64), np.full((steps, E), -1, np.int64)

    def validate():
        call(0, None, None)
        ready.update({t: sb._shapes_upload(*args) for t, args in checked.items()})     # uploads: before the first stretch

    def stretch(a, b):                                    # steps [a, b): behind the reset of step a, if it has one
        if a in ready:
            sb._select_shapes_ready(ready[a])             # out=None: the ring slot the actor reads is not rewritten
        for t in range(a, b):
            if sched is not None and sched[t] >= 0:       # the library's own switch at step t: select_shape's bookkeeping
                sb._note_shapes(np.full(E, sched[t], np.int32), False)
            shape[t] = sb.shape_in_force
            if sb.shape_env_in_force is not None:
                shape_env[t] = sb.shape_env_in_force
        call(b - a, np.ascontiguousarray(sched[a:b]) if sched is not None else None,
             _lib.SwarmEvalOut(ptr(metrics, a), ptr(p, a), ptr(dp, a), ptr(stats, a)))

    _run_stretches(aenv, sb, replay, obs, reset, plan, steps, validate, stretch, "rollout_eval", splits=checked)
    if any(host is None for _, _, host in ready.values()) or any(isinstance(ep, tuple) and ep[1] is None for _, ep, _ in plan.values()):
        shape_env = None                                  # a device index / episode vector: who holds what is not known on the host
    return replay.obs[replay.cur].view(E, N, D), EvalTrace(metrics, p, dp, stats, shape, shape_env)


def _host_array(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def save_eval_results(trace, file_dir, env=0):
    """Write a rollout_eval trace as the files eval_assembly.py:168-174,195-205 writes, for env `env` of the batch, and the
    batch statistics; returns their paths (metrics.pkl, state_data.npz, metrics_batch.npz).

    metrics.pkl      : the reference's list, one dict per step: coverage_rate, uniformity_degree, voronoi_uniformity (floats),
                       et_index, shape_count.  The reference logs shape_count after its increment, so shape_count = the
                       shape index in force + 1 (0 while no switch has happened); with per-env switches (trace.shape_env) it is
                       env `env`'s own shape.
    state_data.npz   : pos, vel [2, N, T] float64 and t_step = T - 1 (the reference saves its loop variable).  Needs a trace
                       recorded with trace_state=True (ValueError otherwise, before anything is written).
    metrics_batch.npz: what the batch adds -- mean, std [T, 3] over the envs, NaN-aware (distribution_uniformity is 0/0 when
                       all minimum distances are equal; a step whose envs are all NaN stays NaN), nan_count [T, 3], and the
                       raw metrics [T, E, 3].
    Waits for the GPU (it reads the trace back)."""
    import os
    import pickle
    import warnings
    if trace.p is None or trace.dp is None:
        raise ValueError("save_eval_results: state_data.npz needs a trace recorded with trace_state=True")
    m = _host_array(trace.metrics).astype(np.float64, copy=False)
    if m.ndim != 3 or m.shape[2] != 3:
        raise ValueError("trace.metrics must be [steps, E, 3]")
    T, E, _ = m.shape
    e = int(env)
    if not 0 <= e < E:
        raise ValueError("env %d outside [0, %d)" % (e, E))
    shape = np.asarray(trace.shape).reshape(-1)
    if shape.shape[0] != T:
        raise ValueError("trace.shape must have one entry per step")
    shape_env = getattr(trace, "shape_env", None)          # per-env switches: env e's own shape
    if shape_env is not None and np.shape(shape_env) != (T, E):
        raise ValueError("trace.shape_env must be [steps, E]")
    p, dp = _host_array(trace.p), _host_array(trace.dp)
    os.makedirs(file_dir, exist_ok=True)
    rows = []
    for t in range(T):
        d = {k: float(m[t, e, j]) for j, k in enumerate(METRIC_KEYS)}
        d["et_index"] = t
        d["shape_count"] = int(shape_env[t, e] if shape_env is not None else shape[t]) + 1
        rows.append(d)
    paths = [os.path.join(file_dir, f) for f in ("metrics.pkl", "state_data.npz", "metrics_batch.npz")]
    with open(paths[0], "wb") as f:
        pickle.dump(rows, f)
    np.savez(paths[1], pos=np.ascontiguousarray(p[:, e].transpose(1, 2, 0)), vel=np.ascontiguousarray(dp[:, e].transpose(1, 2, 0)),
             t_step=T - 1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)            # all-NaN steps: the mean / std stay NaN
        mean, std = np.nanmean(m, axis=1), np.nanstd(m, axis=1)
    np.savez(paths[2], mean=mean, std=std, nan_count=np.isnan(m).sum(axis=1), metrics=m)
    return tuple(paths)


def save_eval_by_shape(trace, file_dir, n_shapes):
    """Write metrics_by_shape.npz for a trace of per-env shapes (rollout_eval with per-env switch entries, or any trace whose
    shape_env is set) and return its path: mean, std [T, S, 3] of the three metrics over the envs that hold shape s at step t,
    NaN-aware exactly as metrics_batch.npz (a NaN metric of an env is left out; all NaN stays NaN), and count [T, S], the
    number of those envs.  A shape nobody holds at a step has count 0 and NaN mean / std.  Envs whose shape is not known
    (-1) are in no group.  Waits for the GPU (it reads the trace back)."""
    import os
    import warnings
    shape_env = getattr(trace, "shape_env", None)
    if shape_env is None:
        raise ValueError("save_eval_by_shape: the trace has no shape_env (a per-env entry's index was a device tensor)")
    m = _host_array(trace.metrics).astype(np.float64, copy=False)
    if m.ndim != 3 or m.shape[2] != 3:
        raise ValueError("trace.metrics must be [steps, E, 3]")
    T, E, _ = m.shape
    shape_env = np.asarray(shape_env)
    if shape_env.shape != (T, E):
        raise ValueError("trace.shape_env must be [steps, E]")
    S = int(n_shapes)
    if S < 1:
        raise ValueError("n_shapes must be >= 1")
    return _save_by_group(m, shape_env, S, file_dir, "metrics_by_shape.npz")


def _save_by_group(m, group, G, file_dir, name):
    """mean, std [T, G, 3] and count [T, G] of the metrics m [T, E, 3] over the envs with group[t, e] == g, NaN-aware, into
    file_dir/name (save_eval_by_shape's file; a group outside [0, G) is in none); returns the path."""
    import os
    import warnings
    T = m.shape[0]
    mean, std = np.full((T, G, 3), np.nan), np.full((T, G, 3), np.nan)
    count = np.zeros((T, G), np.int64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)            # all-NaN groups: the mean / std stay NaN
        for s in range(G):
            held = group == s
            count[:, s] = held.sum(axis=1)
            for t in np.nonzero(count[:, s])[0]:
                mean[t, s], std[t, s] = np.nanmean(m[t, held[t]], axis=0), np.nanstd(m[t, held[t]], axis=0)
    os.makedirs(file_dir, exist_ok=True)
    path = os.path.join(file_dir, name)
    np.savez(path, mean=mean, std=std, count=count)
    return path


def save_eval_by_member(trace, members, file_dir):
    """Write metrics_by_member.npz for a rollout_eval trace of a FusedPolicyBank and return its path: save_eval_by_shape's file
    and NaN rules with the member of an env in place of its shape -- mean, std [T, M, 3] of the three metrics over the envs
    member m acts for (a NaN metric of an env is left out; all NaN stays NaN) and count [T, M], the number of those envs.
    members: an int array [E], the member of every env (FusedPolicyBank.member_of_env(E)), entries in [0, M) with M = its
    maximum + 1, or -1 for an env in no group.  Waits for the GPU (it reads the trace back)."""
    m = _host_array(trace.metrics).astype(np.float64, copy=False)
    if m.ndim != 3 or m.shape[2] != 3:
        raise ValueError("trace.metrics must be [steps, E, 3]")
    T, E, _ = m.shape
    members = np.asarray(members)
    if members.shape != (E,) or members.dtype.kind not in "iu":
        raise ValueError("members must be an int array [E = %d]" % E)
    if members.min() < -1 or members.max() < 0:
        raise ValueError("members must hold member indices >= 0 (or -1 for an env in no group)")
    return _save_by_group(m, np.broadcast_to(members, (T, E)), int(members.max()) + 1, file_dir, "metrics_by_member.npz")
