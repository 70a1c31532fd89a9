"""GPU-resident replay ring — the device counterpart of UniformMemory (reference hirl/utils/buffer.py:11-54).

Rows are 32 fp32 words = one 128-B line: s[13] a[4] s'[13] r done (Transition, buffer.py:8; step_success is kept
in a parallel int8 array because sample() never returns it, buffer.py:47-48).  `total` counts transitions ever
stored; position = total % capacity (buffer.py:36), len = min(total, capacity).
"""
import ctypes

import torch

from .. import _lib


class DeviceReplay:
    def __init__(self, capacity, device="cuda", ordered_slots=False):
        self.capacity = int(capacity)
        self.device = torch.device(device)
        self.ring = torch.zeros((self.capacity, _lib.ROW_WORDS), dtype=torch.float32, device=self.device)
        self.success = torch.zeros(self.capacity, dtype=torch.int8, device=self.device)
        # ordered_slots (opt-in; bench.py): total, then the launch sequence, a status word and one word per row tile of the per-tile acting launches
        # (include/hirl4ucav.h HX_LAYOUT_ORDERED_SLOTS) — those launches then fill the ring in row-tile order, the same for the same inputs
        self.slot_header = torch.zeros(3 + self.capacity // 16, dtype=torch.int64, device=self.device) if ordered_slots else None
        self.total = self.slot_header[:1] if ordered_slots else torch.zeros(1, dtype=torch.int64, device=self.device)

    def slot_status(self):
        """ordered_slots: nonzero once a launch's wait for a lower row tile gave up (its slots may have collided with another tile's); sticky.
        0 without ordered slots.  Synchronises."""
        return 0 if self.slot_header is None else int(self.slot_header[2].item())

    def __len__(self):  # buffer.py:53-54 (host sync: for drivers/tests, not the hot loop)
        return min(int(self.total.item()), self.capacity)

    def fullEnough(self, batchSize):  # buffer.py:50-51
        return len(self) >= batchSize

    def store_rows(self, rows, success=None):
        """Append pre-built rows [k, 32] (expert buffer fill, train_all.py:289-306; tests)."""
        rows = rows.to(self.device, torch.float32).reshape(-1, _lib.ROW_WORDS)
        k = rows.shape[0]
        start = int(self.total.item())
        idx = (torch.arange(k, device=self.device) + start) % self.capacity
        self.ring[idx] = rows
        if success is not None:
            self.success[idx] = success.to(self.device, torch.int8)
        self.total += k
        self.fixed_len = min(start + k, self.capacity)  # host-known live length (tables filled once: expert ring)


HxPer = _lib.STRUCTS["HxPer"]  # the prioritized store's buffers
PER_BLOCK, PER_EPS, PER_MAX_CAPACITY = 1024, 1e-4, 1 << 24
# rows per chunk of score_new's forward launches (include/hirl4ucav.h "Priorities at insert"); from 1,024 rows on a chunk has 128 row tiles per net:
# the forward kernel's wide tiling.  A row's score depends on this value (the launch shape fixes the order of the forward kernel's sums), not on how
# many rows came with it.  Measured (profiles/per_score_new.json): a padded chunk costs what a full one does — 1,024 rows score in
# 39 / 58 / 99 us at chunks of 1,024 / 2,048 / 4,096 —, and larger chunks are cheaper per row — 16,384 rows in 681 / 530 / 436 us.
PER_SCORE_CHUNK = 2048
PER_SCORE_CHUNKS = (1024, 2048, 4096)


def score_chunk_for(max_new):
    """the chunk a loop that scores up to max_new rows per call should use: the smallest of 1,024 / 2,048 / 4,096 that holds them, else 4,096"""
    return next((c for c in PER_SCORE_CHUNKS if int(max_new) <= c), PER_SCORE_CHUNKS[-1])


class PrioritizedReplay(DeviceReplay):
    """The ring with a priority per slot (SacAgent(per=True), SAC/agent.py:112-118; the memory class itself is rltorch's and un-vendored, so the
    store and the draw are this project's definition: include/hirl4ucav.h "Prioritized replay").  prio[slot] = (|delta| + 1e-4)^alpha, 0 = not live;
    bsum = one fixed-order sum per 1,024 slots; pmax = running maximum (new rows enter at it: mark_new); beta <- min(1, beta + beta_annealing)
    per sample call, on the host.  Everything enqueues on the current stream; nothing synchronises."""

    def __init__(self, capacity, device="cuda", ordered_slots=False, alpha=0.6, beta=0.4, beta_annealing=0.0001):
        if int(capacity) > PER_MAX_CAPACITY:
            raise ValueError(f"prioritized replay holds at most 2^24 slots (capacity {int(capacity)}): the sampler scans 16,384 block sums")
        super().__init__(capacity, device, ordered_slots)
        L = _lib.load()
        if L.hx_per_sizeof() != ctypes.sizeof(HxPer):
            raise _lib.HxError(f"ABI mismatch: HxPer is {ctypes.sizeof(HxPer)} bytes here, {L.hx_per_sizeof()} in {_lib.SO_PATH}")
        self.alpha, self.beta, self.beta_annealing = float(alpha), float(beta), float(beta_annealing)
        self.nblocks = (self.capacity + PER_BLOCK - 1) // PER_BLOCK
        self._prio = torch.zeros(self.nblocks * PER_BLOCK, dtype=torch.float32, device=self.device)  # (the padding behind capacity stays 0)
        self.prio = self._prio[:self.capacity]
        self.bsum = torch.zeros(self.nblocks, dtype=torch.float32, device=self.device)
        self._header = torch.zeros(4, dtype=torch.int64, device=self.device)  # word 0: pmax (a float), 1: marked, 2: the launches' ticket
        self.pmax_t = self._header[:1].view(torch.float32)[:1]
        self.pmax_t.fill_(1.0)
        self.marked_t = self._header[1:2]
        self.per = HxPer(self._prio.data_ptr(), self.bsum.data_ptr(), self._header.data_ptr(), self._header[1:].data_ptr(), self._header[2:].data_ptr(),
                         self.total.data_ptr(), self.capacity)
        # score_new: the chunk workspace and the errors of the last call (allocated at the first call, kept), the Philox call word
        self.score_chunk, self.score_calls, self._score_ws, self.errors = PER_SCORE_CHUNK, 0, None, None

    @property
    def pmax(self):  # host sync (drivers / tests)
        return float(self.pmax_t.item())

    @property
    def marked(self):  # host sync
        return int(self.marked_t.item())

    def mark_new(self, max_new=None):
        """every slot stored since the last call enters at pmax.  max_new: an upper bound on their number (the envs stepped); default: the whole ring"""
        _lib.call("hx_per_mark_new", ctypes.byref(self.per), int(max_new) if max_new else self.capacity, _lib.stream_ptr())

    def score_new(self, engine, max_new, eps=None, seed=0):
        """every slot stored since the last call enters at a TD error of its own, |Q1(s, a) - y| with `engine`'s networks as they stand (the
        reference's train_episode, SAC/agent.py:234-246) -> prio = (error + 1e-4)^alpha; a non-finite error enters at pmax.  max_new: an upper bound on
        their number (the envs stepped).  eps [max_new, 4]: the draws of policy.sample(s'), else Philox(seed; row, score_calls).  The errors of the
        rows covered are left in self.errors[:rows].  Enqueues only."""
        max_new = int(max_new)
        if max_new <= 0:
            raise ValueError("score_new: max_new is an upper bound on the rows stored since the last call (> 0)")
        if self._score_ws is None or self._score_ws_chunk != self.score_chunk:
            L = _lib.load()
            words = int(L.hx_per_score_workspace_floats(int(self.score_chunk)))
            if words <= 0:
                raise ValueError(f"score_new: score_chunk is a positive multiple of 16, got {self.score_chunk}")
            self._score_ws, self._score_ws_chunk = torch.zeros(words, dtype=torch.float32, device=self.device), self.score_chunk
        if self.errors is None or self.errors.numel() < max_new:
            self.errors = torch.zeros(max_new, dtype=torch.float32, device=self.device)
        if eps is not None:
            eps = torch.as_tensor(eps, device=self.device).to(torch.float32).contiguous()
            if eps.numel() != max_new * 4:
                raise ValueError(f"score_new: eps is [max_new, 4] = {max_new * 4} draws, got {eps.numel()}")
        self.score_calls += 1
        _lib.call("hx_per_score_new", ctypes.byref(self.per), self.ring.data_ptr(), ctypes.byref(engine.nets), ctypes.byref(engine.hyper), max_new,
                  int(self.score_chunk), self.alpha, _lib.ptr(eps), int(seed), self.score_calls, self._score_ws.data_ptr(), self.errors.data_ptr(),
                  _lib.stream_ptr())

    def set_priorities(self, slots, p):
        """prio[slots] <- p (already raised to alpha)"""
        slots = torch.as_tensor(slots, device=self.device).to(torch.int32).contiguous().reshape(-1)
        p = torch.as_tensor(p, device=self.device).to(torch.float32).contiguous().reshape(-1)
        if slots.numel() != p.numel() or slots.numel() == 0:
            raise ValueError("set_priorities: as many priorities as slots, at least one")
        _lib.call("hx_per_set", ctypes.byref(self.per), slots.data_ptr(), p.data_ptr(), slots.numel(), _lib.stream_ptr())

    def update(self, idx, errors):
        """memory.update_priority(indices, errors) (SAC/agent.py:329-331): prio[idx] <- (|errors| + 1e-4)^alpha, the maximum where a slot repeats"""
        idx = torch.as_tensor(idx, device=self.device).to(torch.int32).contiguous().reshape(-1)
        errors = torch.as_tensor(errors, device=self.device).to(torch.float32).contiguous().reshape(-1)
        if idx.numel() != errors.numel() or idx.numel() == 0:
            raise ValueError("update: as many errors as indices, at least one")
        _lib.call("hx_per_update", ctypes.byref(self.per), idx.data_ptr(), errors.data_ptr(), idx.numel(), self.alpha, _lib.stream_ptr())

    def resum(self):
        _lib.call("hx_per_resum", ctypes.byref(self.per), _lib.stream_ptr())

    def next_beta(self):
        """the beta of this sample call; advances the annealing (host)"""
        b = self.beta
        self.beta = min(1.0, self.beta + self.beta_annealing)
        return b

    def sample_into(self, batch, idx, weights, rows, u=None, seed=0, call=0, beta=None):
        """hx_per_sample: `batch` proportional draws with replacement -> idx (int32), weights, the rows' tile.  u: injected uniforms [batch], else Philox"""
        beta = self.next_beta() if beta is None else float(beta)
        _lib.call("hx_per_sample", ctypes.byref(self.per), self.ring.data_ptr(), int(batch), _lib.ptr(u), int(seed), int(call), beta, idx.data_ptr(),
                  weights.data_ptr(), rows.data_ptr(), _lib.stream_ptr())
        return beta


HxUps = _lib.STRUCTS["HxUps"]  # the success upsampler's buffers
UPS_BLOCK, UPS_MAX_CAPACITY, UPS_BOOST, UPS_BOOST_RANGE = 1024, 1 << 24, 10, (2, 255)


def check_ups_abi():
    L = _lib.load()
    if L.hx_ups_sizeof() != ctypes.sizeof(HxUps):
        raise _lib.HxError(f"ABI mismatch: HxUps is {ctypes.sizeof(HxUps)} bytes here, {L.hx_ups_sizeof()} in {_lib.SO_PATH}")
    return L


def fire_rows(bc_table):
    """the reference's target_indices (HIRL.py:217-219, BC.py:152-158): the rows of an expert table [n, 32] whose fire action (word 16) is 1 -> int32"""
    return torch.nonzero(bc_table[:, 16] == 1).reshape(-1).to(torch.int32)


class SuccessUpsampler:
    """The reference's UniformMemory(upsample=True) draw (buffer.py:18-29, 39-43) beside a DeviceReplay, which stays as it is: a transition whose
    step_success == 1 weighs `boost`, every other 1 (the reference's 1.0 : 0.1 as integers), drawn proportionally WITH replacement and without
    importance weights (include/hirl4ucav.h "Success upsampling").  cnt = the live success rows per 1,024 slots; mark_new(n) behind every acting
    launch keeps it current.  Everything enqueues on the current stream; nothing synchronises but weight_total() and marked."""

    def __init__(self, replay, boost=UPS_BOOST):
        boost = int(boost)
        if not UPS_BOOST_RANGE[0] <= boost <= UPS_BOOST_RANGE[1]:
            raise ValueError(f"upsample boost is {UPS_BOOST_RANGE[0]}..{UPS_BOOST_RANGE[1]} (the weight of a success row against 1), got {boost}")
        if replay.capacity > UPS_MAX_CAPACITY:
            raise ValueError(f"success upsampling holds at most 2^24 slots (capacity {replay.capacity}): the draw scans 16,384 block weights")
        L = check_ups_abi()
        self.replay, self.boost = replay, boost
        self.nblocks = int(L.hx_ups_words(replay.capacity))
        assert self.nblocks == (replay.capacity + UPS_BLOCK - 1) // UPS_BLOCK
        self.cnt = torch.zeros(self.nblocks, dtype=torch.int32, device=replay.device)
        self.marked_t = torch.zeros(1, dtype=torch.int64, device=replay.device)
        self.ups = HxUps(self.cnt.data_ptr(), self.marked_t.data_ptr(), replay.total.data_ptr(), replay.success.data_ptr(), replay.capacity, boost)

    @property
    def marked(self):  # host sync
        return int(self.marked_t.item())

    def mark_new(self, max_new=None):
        """the blocks touched by the rows stored since the last call are recounted.  max_new: an upper bound on their number (the envs stepped);
        default: the whole ring"""
        _lib.call("hx_ups_mark_new", ctypes.byref(self.ups), int(max_new) if max_new else self.replay.capacity, _lib.stream_ptr())

    def recount(self):
        _lib.call("hx_ups_recount", ctypes.byref(self.ups), _lib.stream_ptr())

    def draw_into(self, batch, n_main, idx, rows, x=None, seed=0, call=0, fire=None, bc_table=None, idx_bc=None, bc_rows=None):
        """hx_ups_draw: rows [0, n_main) of idx (int32) / rows <- proportional draws, the rest untouched.  x: injected 64-bit words (int64 tensor,
        n_main of them, two more with `fire`), else Philox(seed; row, call).  fire: int32 indices of bc_table's fire rows -> one row of idx_bc /
        bc_rows is replaced by one of them."""
        draw_call(self, self.replay.ring, batch, n_main, idx, rows, x, seed, call, fire, bc_table, idx_bc, bc_rows)

    def weight_total(self):
        """W = n + (boost - 1) sum(cnt) (host sync: tests)"""
        return min(int(self.replay.total.item()), self.replay.capacity) + (self.boost - 1) * int(self.cnt.sum().item())

    def state(self):
        return {"boost": self.boost, "marked": self.marked}

    def load_state(self, st):
        """after the ring has been restored: the counts are formed again from its labels"""
        if int(st["boost"]) != self.boost:
            raise ValueError(f"snapshot was written under --upsample_boost {st['boost']}, this run has --upsample_boost {self.boost}: resume with the "
                             "value the run was started with")
        self.recount()


def draw_call(upsampler, ring, batch, n_main, idx, rows, x=None, seed=0, call=0, fire=None, bc_table=None, idx_bc=None, bc_rows=None):
    """hx_ups_draw with or without an upsampler (None with n_main = 0: the BC minibatch's fire row alone)"""
    if fire is not None and (fire.dtype != torch.int32 or not fire.is_contiguous() or fire.numel() == 0):
        raise ValueError("fire is a contiguous, non-empty int32 tensor of expert-table rows")
    _lib.call("hx_ups_draw", ctypes.byref(upsampler.ups) if upsampler is not None else None, _lib.ptr(ring), int(batch), int(n_main), _lib.ptr(x),
              int(seed), int(call), _lib.ptr(idx), _lib.ptr(rows), _lib.ptr(fire), fire.numel() if fire is not None else 0, _lib.ptr(bc_table),
              _lib.ptr(idx_bc), _lib.ptr(bc_rows), _lib.stream_ptr())


HxNStep = _lib.STRUCTS["HxNStep"]  # the n-step window's buffers
NSTEP_MAX, NSTEP_FIELDS = _lib.DEFINES["HX_NSTEP_MAX"], _lib.DEFINES["HX_NSTEP_FIELDS"]


class NStepInserter:
    """Truncated n-step returns for the vector loop (SacAgent(multi_step=n); the rule is this project's: include/hirl4ucav.h "n-step returns").  The
    env is built with replay=None; push(env, actions) behind every step keeps up to n pending heads per env and writes finished rows into `replay`
    in the ordinary format, r = sum_k gamma^k r_k and the row's discount folded into the done column, so sample() / learn() run unchanged with the
    one-step gamma.  reset(env) after env.reset().  One call stores at most max_rows = n * num_envs rows.  Everything enqueues on the current stream."""

    def __init__(self, replay, num_envs, n, gamma):
        self.replay, self.num_envs, self.n, self.gamma = replay, int(num_envs), int(n), float(gamma)
        if not 1 <= self.n <= NSTEP_MAX:
            raise ValueError(f"multi_step is 1..{NSTEP_MAX}, got {n}")
        if self.num_envs <= 0:
            raise ValueError(f"NStepInserter: num_envs > 0, got {num_envs}")
        if replay.capacity < self.n * self.num_envs:
            raise ValueError(f"NStepInserter: one step can store n * num_envs = {self.n * self.num_envs} rows, the replay holds {replay.capacity}")
        L = _lib.load()
        if L.hx_nstep_sizeof() != ctypes.sizeof(HxNStep):
            raise _lib.HxError(f"ABI mismatch: HxNStep is {ctypes.sizeof(HxNStep)} bytes here, {L.hx_nstep_sizeof()} in {_lib.SO_PATH}")
        N, k = self.num_envs, NSTEP_FIELDS * self.n * self.num_envs
        words = int(L.hx_nstep_workspace_floats(N, self.n))
        assert words == k + 15 * N
        self.ws = torch.zeros(words, dtype=torch.float32, device=replay.device)  # the whole state: what a snapshot carries
        self.win = self.ws[:k].view(NSTEP_FIELDS, self.n, N)
        self.hc = self.ws[k:k + N].view(torch.int32)            # oldest head's position | pending heads << 8
        self.obs_prev = self.ws[k + N:k + 14 * N].view(13, N)
        self.last_ctr = self.ws[k + 14 * N:].view(torch.int32)
        self.ns = HxNStep(self.win.data_ptr(), self.hc.data_ptr(), self.obs_prev.data_ptr(), self.last_ctr.data_ptr(), N, self.n, self.gamma)

    @property
    def max_rows(self):
        return self.n * self.num_envs

    def reset_arrays(self, obs, episode_ctr):
        _lib.call("hx_nstep_reset", ctypes.byref(self.ns), obs.data_ptr(), episode_ctr.data_ptr(), _lib.stream_ptr())

    def push_arrays(self, obs_new, actions, reward, done, success, episode_ctr):
        r = self.replay
        _lib.call("hx_nstep_push", ctypes.byref(self.ns), obs_new.data_ptr(), actions.data_ptr(), reward.data_ptr(), done.data_ptr(), success.data_ptr(),
                  episode_ctr.data_ptr(), r.ring.data_ptr(), r.success.data_ptr(), r.capacity, r.total.data_ptr(), _lib.stream_ptr())

    def _check(self, env):
        if env.n != self.num_envs:
            raise ValueError(f"NStepInserter was built for {self.num_envs} envs, the env has {env.n}")
        if env.replay is not None:
            raise ValueError("NStepInserter: the env inserts one-step rows itself (replay=...): build it with replay=None")

    def reset(self, env):
        """after env.reset(): every window empty, the next step starts from env.obs"""
        self._check(env)
        self.reset_arrays(env.obs, env.episode_ctr)

    def push(self, env, actions):
        """the step env has just taken with `actions` [num_envs, 4] (fp32, contiguous, on the device), as act_step / env.step left it"""
        self._check(env)
        if actions.dtype != torch.float32 or not actions.is_contiguous() or actions.numel() != self.num_envs * 4:
            raise ValueError("NStepInserter.push: actions are a contiguous fp32 [num_envs, 4] tensor")
        self.push_arrays(env.obs, actions, env.reward, env.done, env.success, env.episode_ctr)

    def state(self):
        return {"n": self.n, "num_envs": self.num_envs, "gamma": self.gamma, "ws": self.ws.cpu().clone()}

    def load_state(self, st):
        if st["n"] != self.n:
            raise ValueError(f"snapshot was written under --multi_step {st['n']}, this run has --multi_step {self.n}: resume with the flag the run was started with")
        if st["num_envs"] != self.num_envs or st["ws"].numel() != self.ws.numel():
            raise ValueError(f"snapshot's n-step windows hold {st['num_envs']} envs, this run {self.num_envs}")
        self.ws.copy_(st["ws"])


def segment_last(done, keep=None):
    """the `last` bytes nstep_relabel takes, for the rows train_all.label_expert keeps of ONE file.  done [k]: their done column; keep [k]: their pair
    indices in the recording (train_all.expert_pair_indices; None: consecutive).  A segment ends at a terminal row, in front of any gap in `keep` (the
    reference skips the pair behind a terminal one) and at the file's last row: no transition spans two files.  -> uint8 numpy [k]"""
    done = np.asarray(done.cpu() if torch.is_tensor(done) else done).reshape(-1) != 0
    last = done.copy()
    if keep is not None:
        keep = np.asarray(keep.cpu() if torch.is_tensor(keep) else keep).reshape(-1).astype(np.int64)
        if keep.shape != done.shape:
            raise ValueError(f"segment_last: {done.size} rows, {keep.size} pair indices")
        last[:-1] |= np.diff(keep) != 1
    if last.size:
        last[-1] = True
    return last.astype(np.uint8)


def nstep_relabel(rows, last, n, gamma):
    """n-step relabelling of a labelled expert table (hx_nstep_label: include/hirl4ucav.h "n-step returns for a labelled expert table").  rows [E, 32]:
    one-step rows in recording order on the device; last [E]: nonzero on the final row of every segment (segment_last).  -> rows_out [E, 32], a new
    tensor: row j holds s, a of row j, r = sum_k gamma^k r_{j+k} over m = min(n, rows left in the segment) steps, s' of row j + m - 1 and the row's
    discount in the done column.  Row j stays row j.  Enqueues only."""
    if not torch.is_tensor(rows) or rows.dtype != torch.float32 or rows.dim() != 2 or rows.shape[1] != _lib.ROW_WORDS or not rows.is_cuda:
        raise ValueError("nstep_relabel: rows is an fp32 [E, 32] tensor on the GPU")
    rows = rows.contiguous()
    E = rows.shape[0]
    last = torch.as_tensor(last).to(device=rows.device, dtype=torch.uint8).contiguous().reshape(-1)
    if last.numel() != E:
        raise ValueError(f"nstep_relabel: {E} rows, {last.numel()} last bytes")
    out = torch.empty_like(rows)
    _lib.call("hx_nstep_label", rows.data_ptr(), last.data_ptr(), E, int(n), float(gamma), out.data_ptr(), _lib.stream_ptr())
    return out


class HostNStep:
    """the same rule on the host for ONE env, one transition per append (SacAgent(multi_step=n).memory): fp32 numpy arithmetic in the kernel's order.
    append -> the finished rows [(row[32], step_success)], oldest first."""

    def __init__(self, n, gamma):
        self.n, self.gamma = int(n), np.float32(gamma)
        self.heads, self.obs_prev = [], None  # a head: [s, a, acc, boot, age, step_success]

    def _row(self, h, s_next, d):
        row = np.zeros(32, np.float32)
        row[0:13], row[13:17], row[17:30], row[30], row[31] = h[0], h[1], s_next, h[2], d
        return row, int(h[5])

    def append(self, state, action, reward, next_state, done, episode_done=None, step_success=0):
        state, next_state = np.asarray(state, np.float32).reshape(13), np.asarray(next_state, np.float32).reshape(13)
        out = []
        one = np.float32(1.0)
        if self.heads and not np.array_equal(state.view(np.uint32), self.obs_prev.view(np.uint32)):
            # the stream broke off (the driver's time-limit step is never appended): the pending heads leave as truncated rows
            out += [self._row(h, self.obs_prev, one - h[3]) for h in self.heads]
            self.heads = []
        self.heads.append([state.copy(), np.asarray(action, np.float32).reshape(4).copy(), np.float32(0.0), np.float32(0.0), 0, step_success])
        r = np.float32(reward)
        for h in self.heads:
            w = one if h[4] == 0 else np.float32(h[3] * self.gamma)
            h[2], h[3], h[4] = np.float32(h[2] + np.float32(w * r)), w, h[4] + 1
        if done:
            out += [self._row(h, next_state, one) for h in self.heads]
            self.heads = []
        elif episode_done:  # the episode ends behind this step without a terminal state: bootstrap from next_state
            out += [self._row(h, next_state, one - h[3]) for h in self.heads]
            self.heads = []
        elif self.heads[0][4] == self.n:
            h = self.heads.pop(0)
            out.append(self._row(h, next_state, one - h[3]))
        self.obs_prev = next_state.copy()
        return out


# ---- reference-API façade -------------------------------------------------------------------------------------------
import random  # noqa: E402
from collections import namedtuple  # noqa: E402

import numpy as np  # noqa: E402,F401  (the reference's drivers obtain `np`, `torch`, `device` from this module's star-export)

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")  # buffer.py:6

Transition = namedtuple("Transition", ("state", "action", "next_state", "reward", "done", "step_success"))  # buffer.py:8


class UniformMemory(DeviceReplay):
    """hirl.utils.buffer.UniformMemory (buffer.py:11-54) over the device ring: store() appends one transition,
    sample() draws without replacement with Python's `random` like the reference and returns the five tuples."""

    def __init__(self, capacity, upsample=False):
        if upsample:
            raise NotImplementedError("priority upsampling is disabled in the reference (HIRL.py:184,189); the vector loop's form of it is "
                                      "SuccessUpsampler beside a DeviceReplay (train_all --buffer_upsample)")
        super().__init__(int(capacity), device)
        self.upsample = False
        self._len = 0
        self.position = 0

    def store(self, state, action, next_state, reward, done, step_success=0):  # buffer.py:20-36
        row = np.zeros(32, np.float32)
        row[0:13], row[13:17], row[17:30] = state, action, next_state
        row[30], row[31] = reward, float(done)
        self.ring[self.position] = torch.from_numpy(row).to(self.device)
        self.success[self.position] = int(step_success)
        self.position = (self.position + 1) % self.capacity
        self._len = min(self._len + 1, self.capacity)
        self.total += 1

    @property
    def memory(self):  # drivers only take len() of it (train_all.py:306,308)
        return range(self._len)

    def __len__(self):
        return self._len

    def fullEnough(self, batchSize):
        return self._len >= batchSize

    def sample_indices(self, batchSize):
        return random.sample(range(self._len), batchSize)  # buffer.py:45

    def sample(self, batchSize):  # buffer.py:38-48
        rows = self.ring[torch.as_tensor(self.sample_indices(batchSize), device=self.device)].cpu().numpy()
        return (tuple(rows[:, 0:13]), tuple(rows[:, 13:17]), tuple(rows[:, 17:30]), tuple(rows[:, 30]), tuple(rows[:, 31]))
