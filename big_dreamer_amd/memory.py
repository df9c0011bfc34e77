"""ExperienceReplay -- same surface and sampling semantics as the reference (src/memory.py:8-104), with
the storage mirrored in HBM and the batch gather done by a HIP kernel (bd_replay_gather), so that
``sample`` returns device tensors without a host-side gather or a bulk H2D copy.

Pixel observations are kept as uint8 (5-bit quantised frames, as the reference stores them) and de-quantised on
the device by bd_replay_gather_pixels; the dequantisation noise is drawn by torch's device generator.

``lanes=N`` splits the ring into N lanes for collecting from N environments at once: lane e owns rows
[e * lane_size, (e + 1) * lane_size), ``append_batch`` writes one transition per lane (one bd_replay_append launch keeps
the mirror in step) and ``_sample_idx`` draws every chunk inside one lane ("Laned replay").

``save`` / ``load`` write and read the filled rows, the counters and the pixel noise state as one uncompressed ``.npz`` of
plain arrays ("Checkpoint and resume").

``device_sampler=True`` moves the draw itself to the device: ``sample`` is ONE bd_replay_sample_gather launch that draws the
chunks from its own Philox stream and gathers them -- nothing from ``np.random``, no index upload ("Device-side
sampling").  ``device_draw`` restates the kernel's draw in Python integers."""
from __future__ import annotations

import numpy as np
import torch

from . import _cabi as cabi
from .checkpoint import atomic_write

_M32 = 0xFFFFFFFF
SAMPLE_STREAM = 12            # csrc/bd_rng.h: the Philox stream id of the device sampler ("replay_sample")


def philox4x32_10(ctr, key):
    """Philox4x32-10 (csrc/bd_rng.h) in Python integers: four counter words, two key words -> four 32-bit words."""
    M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
    c0, c1, c2, c3 = (int(v) & _M32 for v in ctr)
    k0, k1 = (int(v) & _M32 for v in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & _M32, p1 & _M32, ((p0 >> 32) ^ c3 ^ k1) & _M32, p0 & _M32
        k0, k1 = (k0 + W0) & _M32, (k1 + W1) & _M32
    return [c0, c1, c2, c3]


class ExperienceReplay:
    def __init__(self, size, action_size, bit_depth, pixel_observation, observation_size, device, lanes=1,
                 device_sampler=False):
        self.device = torch.device(device)
        self.size = size
        self.lanes = int(lanes)
        if self.lanes < 1 or size // self.lanes < 1:
            raise ValueError(f"ExperienceReplay: {size} rows cannot be split into {lanes} lanes")
        self.lane_size = size // self.lanes     # lane e owns rows [e * lane_size, (e + 1) * lane_size); the rest is unused
        self.pixel_observation = pixel_observation
        self.bit_depth = bit_depth
        if pixel_observation:
            self.observations = np.empty((size, 3, 64, 64), dtype=np.uint8)
        else:
            self.observations = np.empty((size, observation_size), dtype=np.float32)
        self.actions = np.empty((size, action_size), dtype=np.float32)
        self.rewards = np.empty((size,), dtype=np.float32)
        self.nonterminals = np.empty((size, 1), dtype=np.float32)
        self.idx = 0
        self.full = False
        self.steps, self.episodes = 0, 0
        self._dev = None          # device mirror, created lazily / refreshed by sync_device()
        self._dirty = True
        self._out_ring, self._out_i = {}, {}
        self._pix_noise = None
        self._pix_seed, self._pix_step = None, 0
        self._ring = []           # pinned staging buffers for the index upload (async H2D, no host stall)
        self._ring_i = 0
        self._stage = []          # pinned staging buffers of append_batch: [rows | rewards | nonterminals | actions | obs]
        self._stage_i = 0
        self.device_sampler = bool(device_sampler)        # sample() draws on the device (bd_replay_sample_gather)
        self._smp_seed, self._smp_step = None, 0          # its Philox key (drawn at the first device sample) and counter

    # -- reference semantics (src/memory.py:33-49) --
    def append(self, observation, action, reward, done):
        if self.lanes > 1:
            raise ValueError(f"ExperienceReplay.append: this buffer has {self.lanes} lanes, which advance in lock step; "
                             "use append_batch with one transition per lane")
        to_np = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        if self.pixel_observation:
            # postprocess_observation (src/utils.py:320-337): [-0.5, 0.5] float -> quantised uint8
            o = to_np(observation)
            self.observations[self.idx] = np.clip(np.floor((o + 0.5) * 2 ** self.bit_depth) * 2 ** (8 - self.bit_depth),
                                                  0, 2 ** 8 - 1).astype(np.uint8)
        else:
            self.observations[self.idx] = to_np(observation)
        self.actions[self.idx] = to_np(action)
        self.rewards[self.idx] = reward
        self.nonterminals[self.idx] = not done
        if self._dev is not None and not self._dirty:
            i = self.idx
            self._dev["observations"][i].copy_(torch.from_numpy(self.observations[i]))
            self._dev["actions"][i].copy_(torch.from_numpy(self.actions[i]))
            self._dev["rewards"][i] = float(self.rewards[i])
            self._dev["nonterminals"][i] = float(self.nonterminals[i, 0])
        self.idx = (self.idx + 1) % self.size
        self.full = self.full or self.idx == 0
        self.steps, self.episodes = self.steps + 1, self.episodes + (1 if done else 0)

    def append_batch(self, observations, actions, rewards, dones, *, observations_device=None, actions_device=None):
        """One transition per lane: row e of the inputs -- ``(lanes, ...)`` host tensors or arrays, as the environments
        return them -- goes to row ``e * lane_size + idx`` of the host arrays with the arithmetic of ``append``
        (observations are taken as float32), then the shared head advances.

        Where the device mirror exists and is clean, one pinned staging upload ([rows | rewards | nonterminals], plus the
        action / observation rows that are not on the device yet) and ONE bd_replay_append launch write the same rows of the
        mirror.  `observations_device` / `actions_device` are the copies that already sit on the device -- the batch
        uploaded for the encoder (pixels: NCHW in [-0.5, 0.5], quantised by the kernel) and the action the acting step
        returned; the caller vouches that they hold what `observations` / `actions` hold.  Either way the mirror and the host
        arrays hold the same bits afterwards.  The upload and the kernel are enqueued on the current stream
        (``_cabi.stream()``), the stream on which ``sample`` enqueues its gathers, so a later ``sample`` sees the rows in
        order without a synchronisation."""
        to_np = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        n, ls = self.lanes, self.lane_size
        o = np.asarray(to_np(observations), dtype=np.float32)
        a = np.asarray(to_np(actions), dtype=np.float32)
        r = np.asarray(to_np(rewards), dtype=np.float32).reshape(-1)
        d = np.asarray(to_np(dones)).astype(bool).reshape(-1)
        for name, v in (("observations", o), ("actions", a), ("rewards", r), ("dones", d)):
            if v.ndim < 1 or v.shape[0] != n:
                raise ValueError(f"ExperienceReplay.append_batch: {name} has {v.shape[0] if v.ndim else 0} rows, "
                                 f"the buffer has {n} lanes")
        o, a = o.reshape((n,) + self.observations.shape[1:]), a.reshape(n, self.actions.shape[1])
        rows = np.arange(n, dtype=np.int64) * ls + self.idx
        if self.pixel_observation:
            self.observations[rows] = np.clip(np.floor((o + 0.5) * 2 ** self.bit_depth) * 2 ** (8 - self.bit_depth),
                                              0, 2 ** 8 - 1).astype(np.uint8)
        else:
            self.observations[rows] = o
        self.actions[rows] = a
        self.rewards[rows] = r
        self.nonterminals[rows, 0] = ~d
        if self._dev is not None and not self._dirty:
            self._append_device(rows, o, a, observations_device, actions_device)
        self.idx = (self.idx + 1) % ls
        self.full = self.full or self.idx == 0
        self.steps, self.episodes = self.steps + n, self.episodes + int(d.sum())

    def _device_source(self, t, numel, name):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.numel() == numel):
            raise ValueError(f"ExperienceReplay.append_batch: {name} must be a CUDA float32 tensor of {numel} elements")
        return t if t.is_contiguous() else t.contiguous()

    def _append_device(self, rows, o, a, observations_device, actions_device):
        n, A = self.lanes, self.actions.shape[1]
        width = self.observations[0].size
        act_at = 3 * n
        obs_at = (act_at + n * A + 3) // 4 * 4            # 16-byte aligned: the pixel path loads four floats at once
        words = obs_at + n * width
        if not self._stage:
            self._stage = [(torch.empty(words, dtype=torch.int32).pin_memory(),
                            torch.empty(words, dtype=torch.int32, device=self.device),
                            torch.cuda.Event()) for _ in range(4)]
            self._stage_i = 0
        pinned, dev, ev = self._stage[self._stage_i]
        self._stage_i = (self._stage_i + 1) % len(self._stage)
        ev.synchronize()                       # the copy that last used this pinned buffer has completed
        host = pinned.numpy()
        host[:n] = rows
        fhost = host.view(np.float32)
        fhost[n:2 * n] = self.rewards[rows]
        fhost[2 * n:3 * n] = self.nonterminals[rows, 0]
        used = 3 * n
        obs_src = act_src = None
        if actions_device is not None:
            act_src = self._device_source(actions_device, n * A, "actions_device")
        if observations_device is not None:
            obs_src = self._device_source(observations_device, n * width, "observations_device")
        if act_src is None or obs_src is None:             # (the action rows ride along with an observation upload)
            fhost[act_at:act_at + n * A] = a.reshape(-1)
            used = act_at + n * A
        if obs_src is None:
            fhost[obs_at:words] = o.reshape(-1)
            used = words
        dev[:used].copy_(pinned[:used], non_blocking=True)
        ev.record()
        base = dev.data_ptr()
        args = cabi.ReplayAppendArgs()
        args.n, args.size, args.rows = n, self.size, base
        args.obs = obs_src.data_ptr() if obs_src is not None else base + 4 * obs_at
        args.obs_width, args.bit_depth = width, (self.bit_depth if self.pixel_observation else 0)
        args.dst_obs = self._dev["observations"].data_ptr()
        args.act = act_src.data_ptr() if act_src is not None else base + 4 * act_at
        args.A, args.dst_act = A, self._dev["actions"].data_ptr()
        args.reward, args.nonterminal = base + 4 * n, base + 8 * n
        args.dst_reward, args.dst_nonterminal = self._dev["rewards"].data_ptr(), self._dev["nonterminals"].data_ptr()
        cabi.check(cabi.lib.bd_replay_append(args, cabi.stream()))

    def _sample_idx(self, L):
        """src/memory.py:51-68: uniform start, rejected if the chunk crosses the write head.  With lanes the same rule
        inside one uniformly drawn lane (lane-local head, wrap at lane_size)."""
        if self.lanes > 1:
            ls = self.lane_size
            if not self.full and self.idx <= L:
                raise ValueError(f"ExperienceReplay: each of the {self.lanes} lanes holds {self.idx} transitions, a chunk "
                                 f"of {L} needs more (seed more steps, or collect from fewer environments)")
            while True:
                lane = np.random.randint(0, self.lanes)
                start = np.random.randint(0, ls if self.full else self.idx - L)
                local = np.arange(start, start + L) % ls
                if not self.idx in local[1:]:
                    return lane * ls + local
        valid_idx = False
        while not valid_idx:
            idx = np.random.randint(0, self.size if self.full else self.idx - L)
            idxs = np.arange(idx, idx + L) % self.size
            valid_idx = not self.idx in idxs[1:]
        return idxs

    def sync_device(self):
        """(Re)upload the whole buffer to HBM; afterwards append() keeps the mirror in step."""
        self._dev = {k: torch.from_numpy(getattr(self, k)).to(self.device) for k in
                     ("observations", "actions", "rewards", "nonterminals")}
        self._dirty = False

    def mark_dirty(self):
        """Call after writing the numpy arrays directly (e.g. bulk synthetic fill)."""
        self._dirty = True

    # -- checkpoints ("Checkpoint and resume") --
    _ARRAYS = ("observations", "actions", "rewards", "nonterminals")

    def _geometry(self) -> dict:
        """What ``load`` requires to be equal on both sides."""
        return {"size": int(self.size), "lanes": int(self.lanes), "lane_size": int(self.lane_size),
                "bit_depth": int(self.bit_depth), "pixel_observation": int(bool(self.pixel_observation)),
                "observation_width": int(self.observations[0].size), "action_width": int(self.actions.shape[1])}

    def _filled(self, a: np.ndarray) -> np.ndarray:
        """The rows of `a` that hold data: [0, size if full else idx), or per lane [0, lane_size if full else idx) as
        (lanes, k, ...)."""
        if self.lanes == 1:
            return a[:self.size if self.full else self.idx]
        k = self.lane_size if self.full else self.idx
        return a[:self.lanes * self.lane_size].reshape((self.lanes, self.lane_size) + a.shape[1:])[:, :k]

    def save(self, path: str) -> None:
        """Write the buffer to `path` as one uncompressed ``.npz`` of plain arrays: the FILLED rows of the four arrays
        (pixels stay uint8; the uninitialised rest is never written, so the file grows with what has been collected, not
        with ``size``), ``idx`` / ``full`` / ``steps`` / ``episodes``, the geometry ``load`` checks, and the pixel gather's
        noise key and counter.  The host arrays are the truth (the device mirror holds the same bits), so nothing is read
        back from the device.  The write is atomic (checkpoint.atomic_write): `path` holds the old file or the new one."""
        z = {k: np.ascontiguousarray(self._filled(getattr(self, k))) for k in self._ARRAYS}
        z.update({k: np.asarray(v, dtype=np.int64) for k, v in self._geometry().items()})
        z.update(format=np.asarray(1, dtype=np.int64), idx=np.asarray(self.idx, dtype=np.int64),
                 full=np.asarray(bool(self.full)), steps=np.asarray(self.steps, dtype=np.int64),
                 episodes=np.asarray(self.episodes, dtype=np.int64), pix_step=np.asarray(self._pix_step, dtype=np.int64),
                 pix_seed_drawn=np.asarray(self._pix_seed is not None),      # False: keyed at the first pixel sample
                 pix_seed=np.asarray(self._pix_seed or 0, dtype=np.uint64))
        if self.device_sampler:
            z.update(smp_step=np.asarray(self._smp_step, dtype=np.int64), smp_seed_drawn=np.asarray(self._smp_seed is not None),
                     smp_seed=np.asarray(self._smp_seed or 0, dtype=np.uint64))
        atomic_write(path, lambda fh: np.savez(fh, **z))

    def load(self, path: str) -> None:
        """Read a file ``save`` wrote into this buffer, which must have the same ``size``, ``lanes``, widths, ``bit_depth``
        and observation kind (ValueError otherwise: loading into a buffer of another shape is not supported).  Restores the
        rows, the counters and the pixel noise state and calls ``mark_dirty()``: the next ``sample`` uploads the mirror
        again.  Read with ``allow_pickle=False``: nothing from the file is executed."""
        with np.load(path, allow_pickle=False) as z:
            mine = self._geometry()
            theirs = {k: int(z[k]) for k in mine}
            if theirs != mine:
                diff = {k: (mine[k], theirs[k]) for k in mine if mine[k] != theirs[k]}
                raise ValueError(f"ExperienceReplay.load: {path} was saved from a buffer of another shape "
                                 f"(this buffer, file): {diff}")
            idx, full = int(z["idx"]), bool(z["full"])
            head = self.lane_size if self.lanes > 1 else self.size
            if not 0 <= idx < head:
                raise ValueError(f"ExperienceReplay.load: {path} has idx={idx}, this buffer's head runs in [0, {head})")
            old, (self.idx, self.full) = (self.idx, self.full), (idx, full)
            for k in self._ARRAYS:
                dst, src = self._filled(getattr(self, k)), z[k]
                if src.shape != dst.shape or src.dtype != dst.dtype:
                    self.idx, self.full = old
                    raise ValueError(f"ExperienceReplay.load: {path}: {k} is {src.dtype}{src.shape}, this buffer's filled "
                                     f"rows are {dst.dtype}{dst.shape}")
                dst[...] = src
            self.steps, self.episodes = int(z["steps"]), int(z["episodes"])
            self._pix_step = int(z["pix_step"])
            self._pix_seed = int(z["pix_seed"]) if bool(z["pix_seed_drawn"]) else None
            drawn = "smp_seed_drawn" in z.files and bool(z["smp_seed_drawn"])      # a file without the keys: (undrawn, 0)
            self._smp_seed = int(z["smp_seed"]) if drawn else None
            self._smp_step = int(z["smp_step"]) if "smp_step" in z.files else 0
        self.mark_dirty()

    def _upload_indices(self, vec: np.ndarray) -> torch.Tensor:
        """Async H2D of the gather indices through a ring of pinned buffers, so that the host can run
        ahead of the GPU (a pageable copy would wait for all queued kernels of the previous step)."""
        if not self._ring or self._ring[0][0].numel() != vec.size:
            self._ring = [(torch.empty(vec.size, dtype=torch.int64).pin_memory(),
                           torch.empty(vec.size, dtype=torch.int64, device=self.device),
                           torch.cuda.Event()) for _ in range(4)]
            self._ring_i = 0
        pinned, dev, ev = self._ring[self._ring_i]
        self._ring_i = (self._ring_i + 1) % len(self._ring)
        ev.synchronize()                       # the copy that last used this pinned buffer has completed
        pinned.copy_(torch.from_numpy(vec))
        dev.copy_(pinned, non_blocking=True)
        ev.record()
        return dev

    def _out(self, key: str, numel: int) -> torch.Tensor:
        """Output buffers come from a ring of four persistent allocations per array, so that the kernels downstream
        see a small repeating set of operand addresses (descriptor tables and graphs can be reused) while a batch
        stays valid for the next three `sample` calls -- the engine's pipeline holds one for at most two."""
        ring = self._out_ring.setdefault((key, numel), [])
        if len(ring) < 4:
            ring.append(torch.empty(numel, dtype=torch.float32, device=self.device))
            return ring[-1]
        i = self._out_i.get((key, numel), 0)
        self._out_i[(key, numel)] = (i + 1) % 4
        return ring[i]

    # -- device-side sampling ("Device-side sampling") --
    def _draw_geometry(self, n, L):
        """(R, n_valid) of a draw of n chunks of L rows: the ring a chunk lives in and the number of accepted starts.
        ValueError where the host route raises one (its message), or would never find a chunk."""
        n, L = int(n), int(L)
        R = self.lane_size if self.lanes > 1 else self.size
        if not 1 <= n <= 4096:
            raise ValueError(f"ExperienceReplay: the device sampler draws 1 to 4096 sequences per call (got {n})")
        if L < 1:
            raise ValueError(f"ExperienceReplay: a chunk has at least one row (got L={L})")
        if L > R:
            raise ValueError(f"ExperienceReplay: a chunk of {L} does not fit a ring of {R} rows")
        if not self.full and self.idx <= L:
            if self.lanes > 1:
                raise ValueError(f"ExperienceReplay: each of the {self.lanes} lanes holds {self.idx} transitions, a chunk "
                                 f"of {L} needs more (seed more steps, or collect from fewer environments)")
            raise ValueError(f"ExperienceReplay: the buffer holds {self.idx} transitions, a chunk of {L} needs more")
        return R, (R - L + 1 if self.full else self.idx - L)

    def device_draw(self, n, L, step=None, seed=None) -> np.ndarray:
        """The rows bd_replay_sample_gather draws for (seed, step), restated in Python integers: int64 [L * n], time-major
        (element t * n + b).  Needs no device.  `step` None: the current counter, which is not advanced; `seed` None: the
        buffer's key (``int(torch.initial_seed())`` where it has not been drawn yet, which is what the first device sample
        will draw).  Sequence b: x = philox4x32_10((b, 0, 12, step), seed); lane = x[0] * lanes >> 32;
        u = (x[2] | x[3] << 32) * n_valid >> 64; start = u (not full) or (idx + u) mod R (full)."""
        n, L = int(n), int(L)
        R, n_valid = self._draw_geometry(n, L)
        step = self._smp_step if step is None else int(step)
        if seed is None:
            seed = self._smp_seed if self._smp_seed is not None else int(torch.initial_seed())
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        out = np.empty((L, n), dtype=np.int64)
        for b in range(n):
            x = philox4x32_10((b, 0, SAMPLE_STREAM, step & _M32), (seed & _M32, seed >> 32))
            out[:, b] = self._chunk_rows((x[0] * self.lanes) >> 32, ((x[2] | x[3] << 32) * n_valid) >> 64, L)
        return out.reshape(-1)

    def _chunk_rows(self, lane, u, L):
        """Rows of the chunk that the uniform draws (lane, u in [0, n_valid)) select."""
        R = self.lane_size if self.lanes > 1 else self.size
        start = (self.idx + u) % R if self.full else u
        return [lane * R + (start + t) % R for t in range(L)]

    def _sample_device(self, n, L, _idx_out=None):
        n, L = int(n), int(L)
        self._draw_geometry(n, L)
        if _idx_out is not None and not (isinstance(_idx_out, torch.Tensor) and _idx_out.is_cuda and _idx_out.dtype == torch.int64
                                         and _idx_out.is_contiguous() and _idx_out.numel() == L * n):
            raise ValueError(f"ExperienceReplay.sample: _idx_out must be a contiguous CUDA int64 tensor of {L * n} elements")
        if self._dev is None or self._dirty:
            self.sync_device()
        if self._smp_seed is None:
            self._smp_seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        px = self.pixel_observation
        if px and self._pix_seed is None:
            self._pix_seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        dev = self._dev
        O, A = self.observations[0].size, self.actions.shape[1]
        a = cabi.ReplaySampleArgs()
        a.obs, a.act = dev["observations"].data_ptr(), dev["actions"].data_ptr()
        a.reward, a.nonterminal = dev["rewards"].data_ptr(), dev["nonterminals"].data_ptr()
        a.obs_width, a.A, a.size, a.lanes, a.lane_size = O, A, self.size, self.lanes, self.lane_size
        a.idx, a.full, a.n, a.L, a.bit_depth = self.idx, int(self.full), n, L, (self.bit_depth if px else 0)
        a.seed, a.step = self._smp_seed, self._smp_step & _M32
        a.pix_seed, a.pix_step = (self._pix_seed, self._pix_step) if px else (0, 0)
        obs = self._out("pixels" if px else "observations", L * n * O)
        act, rew, non = self._out("actions", L * n * A), self._out("rewards", L * n), self._out("nonterminals", L * n)
        a.dst_obs, a.dst_act, a.dst_reward, a.dst_nonterminal = obs.data_ptr(), act.data_ptr(), rew.data_ptr(), non.data_ptr()
        if _idx_out is not None:
            a.idx_out = _idx_out.data_ptr()
        cabi.check(cabi.lib.bd_replay_sample_gather(a, cabi.stream()))
        self._smp_step += 1
        if px:
            self._pix_step += 1
        return [obs.view(L, n, 3, 64, 64) if px else obs.view(L, n, -1), act.view(L, n, -1), rew.view(L, n), non.view(L, n, 1)]

    def sample(self, n, L, _idx_out=None):
        """Time-major batch [obs (L,n,O), actions (L,n,A), rewards (L,n), nonterminals (L,n,1)] on the device
        (src/memory.py:70-104).  With ``device_sampler`` the chunks are drawn on the device too (one launch, nothing from
        ``np.random``); `_idx_out` (CUDA int64 [L * n]) then receives the rows drawn."""
        if self.device_sampler:
            if self.device.type != "cuda":
                raise RuntimeError("ExperienceReplay.sample: the HIP path needs a GPU device (no CPU fallback)")
            return self._sample_device(n, L, _idx_out)
        if _idx_out is not None:
            raise ValueError("ExperienceReplay.sample: _idx_out belongs to the device sampler (device_sampler=True)")
        idxs = np.asarray([self._sample_idx(L) for _ in range(n)])
        vec = np.ascontiguousarray(idxs.transpose().reshape(-1)).astype(np.int64)
        if self.device.type != "cuda":
            raise RuntimeError("ExperienceReplay.sample: the HIP path needs a GPU device (no CPU fallback)")
        if self._dev is None or self._dirty:
            self.sync_device()
        vidx = self._upload_indices(vec)
        out = []
        if self.pixel_observation:
            src = self._dev["observations"]
            pixels = 3 * 64 * 64
            # dequantisation noise (rand_like, src/utils.py:317) drawn inside the gather kernel: Philox keyed by the torch
            # seed at the first sample, counter = sample index (no noise tensor, no library RNG launch per step)
            if self._pix_seed is None:
                self._pix_seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
            dst = self._out("pixels", L * n * pixels)
            cabi.check(cabi.lib.bd_replay_gather_pixels_rng(src.data_ptr(), vidx.data_ptr(), L * n, pixels, self.bit_depth,
                                                            self._pix_seed, self._pix_step, dst.data_ptr(), cabi.stream()))
            self._pix_step += 1
            out.append(dst.view(L, n, 3, 64, 64))
        for key, shape in (("observations", (L, n, -1)), ("actions", (L, n, -1)), ("rewards", (L, n)),
                           ("nonterminals", (L, n, 1))):
            if key == "observations" and self.pixel_observation:
                continue
            src = self._dev[key]
            width = src.numel() // src.shape[0]
            dst = self._out(key, L * n * width)
            cabi.check(cabi.lib.bd_replay_gather(src.data_ptr(), vidx.data_ptr(), L * n, width, dst.data_ptr(),
                                                 cabi.stream()))
            out.append(dst.view(*shape))
        return out
