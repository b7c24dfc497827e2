"""Device replay for the batched train-ddpg-cnn.py rollout.

duckietown_rl/utils.py:18-57 keeps a list of transitions; a full buffer pops
a uniformly drawn list position and appends, and ``sample`` draws list
positions uniformly.  List order is therefore unobservable in distribution,
and the buffer is restated in slot form, with every draw a pure function of a
serial number:

  * transition ``s`` (the 0-based count of every add) takes slot ``s`` while
    ``s < max_size``; later it evicts slot ``(w * max_size) >> 32``, ``w`` =
    word 0 of ``philox4x32_10((lo32(s), hi32(s), 0, 'EVIC'), key_of(seed))``;
  * of two adds of one batch to one slot the later keeps it, as sequential
    adds would leave it (a batch may evict a transition it added itself);
  * draw ``d`` (the count of every draw) reads slot ``(w * len) >> 32`` with
    the block tagged 'SMPL': slots fill in order and are never vacated.

A transition is stored as six palette-index byte frames (state 0-2,
next_state 3-5, newest first; 19,200 B each, written once, straight from the
rollout's ring) plus action, reward and done: 115,216 B instead of
ddpg.ReplayBuffer's 460,816 B.  ``gather`` decodes the frames through the
renderer's grey table, bit for bit what dt_stack_take gives the actor.

Every operation is stated twice, as cnn_rollout's SubstepBook / FusedBook
are: with torch ops (any device) and as one HIP launch (include/dtreplay.h);
the two agree bit for bit (tests/test_gpu_cnn_replay.py).  ``added`` and
``drawn`` are host integers: nothing here reads the device back.
"""
import ctypes

import torch

from aido1_amd import _lib
from aido1_amd.render import H, W, palette_gray

TAG_EVICT = 0x45564943      # 'EVIC'
TAG_SAMPLE = 0x534D504C     # 'SMPL'
_MASK = 0xFFFFFFFF
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def _mulhilo(m, c):
    """(hi, lo) 32-bit halves of m * c for a constant m < 2^32 and an int64
    tensor c of values < 2^32, without leaving int64's positive range: c is
    split into 16-bit halves, so every product stays below 2^48."""
    ph = m * (c >> 16)
    t = ((ph & 0xFFFF) << 16) + m * (c & 0xFFFF)
    return (ph >> 16) + (t >> 32), t & _MASK


def philox_word0(serials, tag, seed):
    """Word 0 of philox4x32_10((lo32(s), hi32(s), 0, tag), (lo32(seed),
    hi32(seed))) for an int64 tensor of serials: Random123's rounds (the
    spawn path's generator, csrc/dtsim_common.h) in int64 torch ops."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & _MASK, seed >> 32
    c0, c1 = serials & _MASK, (serials >> 32) & _MASK
    c2 = torch.zeros_like(serials)
    c3 = torch.full_like(serials, tag)
    for r in range(10):
        if r:
            k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
        hi0, lo0 = _mulhilo(_M0, c0)
        hi1, lo1 = _mulhilo(_M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
    return c0


class CnnReplay:
    """ddpg.ReplayBuffer's role for CnnRollout.collect and DDPG.train, on the
    device.  fused: the HIP kernels (default on a GPU) or the torch ops
    (default elsewhere).  dtype: what ``gather`` returns (float32 stacks are
    converted when the policy trains in another precision).

    ``_s`` = (frames u8 [max_size, 6, 120, 160], action f32 [max_size, 2],
    reward f32 [max_size], done f32 [max_size]); ``owner`` i64 [max_size]: the
    serial each slot holds, plus one (0: never written)."""

    def __init__(self, max_size, device=None, seed=0, fused=None, dtype=torch.float32):
        self.max_size = int(max_size)
        if not 1 <= self.max_size < 2 ** 31:
            raise ValueError('max_size must be in [1, 2^31)')
        self.device = dev = torch.device(device) if device is not None else (
            torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available()
            else torch.device('cpu'))
        self.fused = dev.type == 'cuda' if fused is None else bool(fused)
        if self.fused and dev.type != 'cuda':
            raise ValueError('fused=True needs a GPU: the kernels have no host form')
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.dtype = dtype
        self.added = 0          # every transition ever added
        self.drawn = 0          # every sample ever drawn
        m = self.max_size
        self._s = (torch.zeros(m, 6, H, W, dtype=torch.uint8, device=dev),
                   torch.zeros(m, 2, dtype=torch.float32, device=dev),
                   torch.zeros(m, dtype=torch.float32, device=dev),
                   torch.zeros(m, dtype=torch.float32, device=dev))
        self.owner = torch.zeros(m, dtype=torch.int64, device=dev)
        self.rows = None        # the open claim: claim() .. commit()

    def __len__(self):
        return min(self.added, self.max_size)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def storage_serials(self):
        """The serial each slot holds (-1: never written)."""
        return self.owner - 1

    # ---- adding -------------------------------------------------------------------------
    def claim(self, n):
        """The slots of the next n transitions (serials added .. added + n - 1):
        int64 [n], -1 for a transition that a later one of the batch evicts.
        Open until commit()."""
        n = int(n)
        rows = torch.empty(n, dtype=torch.int64, device=self.device)
        if self.fused:
            _lib.call('dt_replay_claim', n, self.added, self.max_size, self.seed,
                      self.owner.data_ptr(), rows.data_ptr(), self._stream())
        elif n:
            s = torch.arange(self.added, self.added + n, dtype=torch.int64, device=self.device)
            slots = torch.where(s < self.max_size, s,
                                (philox_word0(s, TAG_EVICT, self.seed) * self.max_size) >> 32)
            # serials grow with the env index: an add loses to any later add of its slot
            lost = (slots[:, None] == slots[None, :]).triu(1).any(1)
            rows.copy_(torch.where(lost, torch.full_like(slots, -1), slots))
            self.owner[slots[~lost]] = s[~lost] + 1
        self.rows = rows
        return rows

    def store(self, ring, order, mask, half):
        """The stacks of the open claim: frames[rows[e], 3 * half + j] =
        ring[e, order[j]] for the envs with mask[e] != 0 (None: all) that kept
        their slot.  ring: uint8 [n, slots, 120, 160] palette-index frames;
        half 0: state, 1: next_state."""
        rows, frames = self.rows, self._s[0]
        n = rows.numel()
        if ring.dtype != torch.uint8 or not ring.is_contiguous() or ring.dim() != 4 or \
                tuple(ring.shape[2:]) != (H, W) or ring.shape[0] != n:
            raise ValueError('store needs a contiguous uint8 [n, slots, %d, %d] index ring' % (H, W))
        if half not in (0, 1):
            raise ValueError('half is 0 (state) or 1 (next_state)')
        order = [int(o) for o in order]
        if self.fused:
            assert mask is None or (mask.dtype == torch.uint8 and mask.is_contiguous()
                                    and mask.numel() == n)
            _lib.call('dt_stack_store', ring.data_ptr(), n, ring.shape[1],
                      (ctypes.c_int32 * 3)(*order), mask.data_ptr() if mask is not None else None,
                      rows.data_ptr(), int(half), frames.data_ptr(), self._stream())
            return
        if any(not 0 <= o < ring.shape[1] for o in order) or len(order) != 3:
            raise ValueError('order names three ring slots')
        sel = rows >= 0
        if mask is not None:
            sel = sel & (mask != 0)
        frames[rows[sel], 3 * half:3 * half + 3] = ring[sel][:, order]

    def commit(self, action, repeat_reward, done_float):
        """The scalars of the open claim (action f32 [n, 2], repeat_reward f64
        [n] rounded to float32 as ddpg.ReplayBuffer stores it, done_float f32
        [n]); closes the claim and advances ``added``."""
        rows = self.rows
        n = rows.numel()
        _, a, r, d = self._s
        for t, dt, shape in ((action, torch.float32, (n, 2)), (repeat_reward, torch.float64, (n,)),
                             (done_float, torch.float32, (n,))):
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError('commit: expected a contiguous %s %s tensor' % (dt, shape))
        if self.fused:
            _lib.call('dt_replay_commit', n, rows.data_ptr(), action.data_ptr(),
                      repeat_reward.data_ptr(), done_float.data_ptr(), a.data_ptr(),
                      r.data_ptr(), d.data_ptr(), self._stream())
        else:
            sel = rows >= 0
            a[rows[sel]] = action[sel]
            r[rows[sel]] = repeat_reward[sel].float()
            d[rows[sel]] = done_float[sel]
        self.added += n
        self.rows = None
        return rows

    # ---- sampling -----------------------------------------------------------------------
    def sample_slots(self, batch_size=100):
        """The slots of draws drawn .. drawn + batch_size - 1: a device int64
        tensor, no host synchronisation."""
        b, length = int(batch_size), len(self)
        if length < 1:
            raise ValueError('sample_slots on an empty buffer')
        if self.fused:
            idx = torch.empty(b, dtype=torch.int64, device=self.device)
            _lib.call('dt_replay_draw', b, self.drawn, length, self.seed, idx.data_ptr(),
                      self._stream())
        else:
            d = torch.arange(self.drawn, self.drawn + b, dtype=torch.int64, device=self.device)
            idx = (philox_word0(d, TAG_SAMPLE, self.seed) * length) >> 32
        self.drawn += b
        return idx

    def gather(self, slots, flat=False):
        """ddpg.ReplayBuffer.gather's dict for int64 slots (each in [0,
        len(self)), unchecked): 'state' / 'next_state' [b, 3, 120, 160] (on a
        GPU in channels-last memory, what DDPG._iteration asks for; flat: [b,
        57600] planes), 'action' [b, 2], 'reward' and 'done' [b, 1]."""
        idx = slots if torch.is_tensor(slots) else torch.as_tensor(slots, dtype=torch.int64)
        idx = idx.to(device=self.device, dtype=torch.int64).contiguous()
        b = idx.numel()
        frames, a, r, d = self._s
        nhwc = self.device.type == 'cuda' and not flat
        fmt = torch.channels_last if nhwc else torch.contiguous_format
        if self.fused:
            kw = dict(dtype=torch.float32, device=self.device)
            st = torch.empty(b, 3, H, W, memory_format=fmt, **kw)
            nx = torch.empty(b, 3, H, W, memory_format=fmt, **kw)
            act, rew, done = torch.empty(b, 2, **kw), torch.empty(b, 1, **kw), torch.empty(b, 1, **kw)
            _lib.call('dt_cnn_replay_gather', b, idx.data_ptr(), frames.data_ptr(), a.data_ptr(),
                      r.data_ptr(), d.data_ptr(), int(nhwc), st.data_ptr(), nx.data_ptr(),
                      act.data_ptr(), rew.data_ptr(), done.data_ptr(), self._stream())
        else:
            pal = palette_gray(self.device)
            both = pal[frames.index_select(0, idx).long()]
            st = both[:, :3].contiguous(memory_format=fmt)
            nx = both[:, 3:].contiguous(memory_format=fmt)
            act = a.index_select(0, idx)
            rew = r.index_select(0, idx).reshape(-1, 1)
            done = d.index_select(0, idx).reshape(-1, 1)
        if flat:
            st, nx = st.flatten(1), nx.flatten(1)
        out = {'state': st, 'next_state': nx, 'action': act, 'reward': rew, 'done': done}
        if self.dtype != torch.float32:
            out = {k: v.to(self.dtype) for k, v in out.items()}
        return out

    def sample(self, batch_size=100, flat=False):
        return self.gather(self.sample_slots(batch_size), flat)
