"""The device replay of the batched train-ddpg-cnn.py rollout, without a GPU
(aido1_amd/cnn_replay.py, include/dtreplay.h): the slot rules' CPU
restatement (tests/cnn_replay_ref.py) against a plain sequential loop and for
uniformity, CnnReplay's torch path against the restatement, DDPG.train on it,
and the entry points' host-side argument checks."""
import ctypes
import itertools

import numpy as np
import torch

import cnn_replay_ref as R

SEED = 123
BATCHES = (1, 7, 33, 300)


def test_restatement_equals_a_sequential_loop():
    """max_size 16, batches of 1, 7, 33 and 300 from added = 0: rows_of equals
    what single adds in serial order leave in a dict slot -> serial (an add
    whose slot the dict maps to a later serial of its batch lost it).  Some
    batch must claim a slot twice; 33 adds to a full buffer hit 15 distinct
    slots, so the later-wins rule is exercised."""
    m, held, added, twice = 16, {}, 0, 0
    for n in BATCHES:
        mine = []
        for i in range(n):
            s = added + i
            if s < m:
                sl = s
            else:
                w = R.philox4x32_10((s & 0xFFFFFFFF, s >> 32, 0, 0x45564943), R.key_of(SEED))[0]
                sl = (w * m) >> 32
            assert 0 <= sl < m
            held[sl] = s
            mine.append((sl, s))
        slots = R.slots_of(added, n, m, SEED)
        assert slots == [sl for sl, _ in mine]
        assert R.rows_of(added, n, m, SEED) == [sl if held[sl] == s else -1 for sl, s in mine]
        twice += len(slots) - len(set(slots))
        added += n
        want = [held.get(sl, -1) for sl in range(m)]
        assert R.serials_after(BATCHES[:BATCHES.index(n) + 1], m, SEED) == want
    assert twice > 0
    full = R.slots_of(16, 33, m, SEED)           # 33 adds to a full buffer
    assert len(set(full)) == 15
    assert sum(r >= 0 for r in R.rows_of(16, 33, m, SEED)) == 15


def _chi_square(values, bins):
    counts = np.bincount(np.asarray(values), minlength=bins)
    assert counts.size == bins
    e = len(values) / bins
    return float(((counts - e) ** 2 / e).sum())


def test_restatement_is_uniform():
    """Seed 123.  12,800 evictions (serials 64 .. 12,863) into 64 slots:
    chi-square 56.78 against 103.4, the 99.9 % point at 63 degrees of freedom;
    9,600 draws over len 48: 35.86 against 82.7 (47 degrees)."""
    ev = _chi_square(R.slots_of(64, 12800, 64, SEED), 64)
    dr = _chi_square(R.draws_of(0, 9600, 48, SEED), 48)
    print('chi-square: evictions %.2f, draws %.2f' % (ev, dr))
    assert ev < 103.4
    assert dr < 82.7


def test_torch_philox_equals_the_oracle():
    """cnn_replay.philox_word0 (int64 torch ops, 16-bit split products)
    against oracle/philox_ref.py on serials around 2^16, 2^32 and 2^40 and
    two seeds with high key words."""
    from aido1_amd.cnn_replay import TAG_EVICT, TAG_SAMPLE, philox_word0
    assert (TAG_EVICT, TAG_SAMPLE) == (R.TAG_EVICT, R.TAG_SAMPLE)
    serials = [0, 1, 2, 65535, 65536, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 40 + 7, 2 ** 62]
    for seed, tag in itertools.product((SEED, 0xFEDCBA9876543210), (TAG_EVICT, TAG_SAMPLE)):
        got = philox_word0(torch.tensor(serials, dtype=torch.int64), tag, seed).tolist()
        want = [R.philox4x32_10((s & 0xFFFFFFFF, s >> 32, 0, tag), R.key_of(seed))[0]
                for s in serials]
        assert got == want, (seed, tag)


def _fill(rp, batches, g, model):
    """Adds the batches to rp from random rings, orders, masks and scalars;
    model: slot -> (frames u8 [6, 120, 160], action, reward f32, done)."""
    perms = list(itertools.permutations(range(3)))
    for k, n in enumerate(batches):
        added = rp.added
        rings = [torch.randint(0, 8, (n, 3, 120, 160), generator=g).to(torch.uint8)
                 for _ in range(3)]
        orders = [perms[(k + j) % 6] for j in range(3)]
        mask = (torch.rand(n, generator=g) < 0.5).to(torch.uint8)
        action = torch.rand(n, 2, generator=g) * 2 - 1
        reward = torch.randn(n, dtype=torch.float64, generator=g)
        done = (torch.rand(n, generator=g) < 0.3).float()
        rows = rp.claim(n)
        want_rows = R.rows_of(added, n, rp.max_size, rp.seed)
        assert rows.tolist() == want_rows
        rp.store(rings[0], orders[0], None, 0)
        rp.store(rings[1], orders[1], mask, 1)
        rp.store(rings[2], orders[2], 1 - mask, 1)
        assert rp.commit(action, reward, done) is rows
        assert rp.added == added + n
        for e, row in enumerate(want_rows):
            if row >= 0:
                nxt = rings[1] if mask[e] else rings[2]
                o = orders[1] if mask[e] else orders[2]
                model[row] = (torch.cat([rings[0][e, list(orders[0])], nxt[e, list(o)]]),
                              action[e], reward[e].float(), done[e])


def test_torch_path_equals_the_restatement():
    """CnnReplay(16, 'cpu'): batches of 1, 7 and 33 (the last evicts, also its
    own transitions): rows, storage_serials, every stored byte and scalar, the
    gather's decode and layout, and the draws."""
    from aido1_amd.cnn_replay import CnnReplay
    from aido1_amd.render import palette_gray
    g = torch.Generator().manual_seed(5)
    rp = CnnReplay(16, device='cpu', seed=SEED)
    assert not rp.fused and len(rp) == 0
    assert rp._s[0].dtype == torch.uint8 and tuple(rp._s[0].shape) == (16, 6, 120, 160)
    model = {}
    _fill(rp, BATCHES[:3], g, model)
    assert len(rp) == 16 and rp.added == 41
    assert rp.storage_serials().tolist() == R.serials_after(BATCHES[:3], 16, SEED)
    slots = sorted(model)
    assert slots == list(range(16))
    b = rp.gather(slots + [3, 3])
    pal = palette_gray('cpu')
    want = torch.stack([model[s][0] for s in slots + [3, 3]])
    assert torch.equal(rp._s[0], want[:16])
    assert b['state'].dtype == torch.float32 and tuple(b['state'].shape) == (18, 3, 120, 160)
    assert torch.equal(b['state'], pal[want[:, :3].long()])
    assert torch.equal(b['next_state'], pal[want[:, 3:].long()])
    assert torch.equal(b['action'], torch.stack([model[s][1] for s in slots + [3, 3]]))
    assert torch.equal(b['reward'], torch.stack([model[s][2] for s in slots + [3, 3]]).view(-1, 1))
    assert torch.equal(b['done'], torch.stack([model[s][3] for s in slots + [3, 3]]).view(-1, 1))
    flat = rp.gather([2, 9], flat=True)
    assert tuple(flat['state'].shape) == (2, 3 * 120 * 160)
    assert torch.equal(flat['next_state'], pal[want[[2, 9], 3:].long()].flatten(1))
    d1, d2 = rp.sample_slots(5), rp.sample_slots(300)
    assert d1.dtype == torch.int64 and rp.drawn == 305
    assert d1.tolist() + d2.tolist() == R.draws_of(0, 305, 16, SEED)
    s = rp.sample(4)
    assert rp.drawn == 309 and tuple(s['state'].shape) == (4, 3, 120, 160)


def test_ddpg_trains_on_it_on_the_cpu():
    """DDPG(device='cpu').train(CnnReplay, 2, batch_size=4) as it stands: it
    draws through sample_slots (drawn advances by 8) and moves the weights."""
    from aido1_amd.cnn_replay import CnnReplay
    from aido1_amd.ddpg import DDPG
    torch.manual_seed(3)
    g = torch.Generator().manual_seed(9)
    rp = CnnReplay(8, device='cpu', seed=SEED)
    _fill(rp, (8,), g, {})
    agent = DDPG(None, 2, 1.0, 'cnn', device='cpu', log=None)
    before = [p.detach().clone() for p in agent.actor.parameters()] + \
        [p.detach().clone() for p in agent.critic.parameters()]
    agent.train(rp, 2, batch_size=4)
    after = list(agent.actor.parameters()) + list(agent.critic.parameters())
    assert rp.drawn == 8
    assert all(torch.isfinite(p).all() for p in after)
    assert any(not torch.equal(a, b) for a, b in zip(after, before))
    assert torch.isfinite(agent.critic_loss) and torch.isfinite(agent.actor_loss)


def test_entry_points_refuse_bad_arguments_on_the_host():
    """Every new entry point returns DT_E_ARG before any launch (no device
    needed; the non-NULL pointers are never read): n < 0, a NULL pointer, a
    misaligned store, an order outside [0, slots), sizes out of range."""
    from aido1_amd import _lib
    L = _lib.lib()
    ARG, p, q = -1, 0x10000, 0x10008           # p 16-B aligned, q not
    order = (ctypes.c_int32 * 3)(0, 1, 2)
    past = (ctypes.c_int32 * 3)(0, 1, 3)
    below = (ctypes.c_int32 * 3)(-1, 1, 2)
    cases = [
        ('dt_replay_claim', (-1, 0, 16, SEED, p, p, None)),
        ('dt_replay_claim', (4, -1, 16, SEED, p, p, None)),
        ('dt_replay_claim', (4, 0, 0, SEED, p, p, None)),
        ('dt_replay_claim', (4, 0, 2 ** 31, SEED, p, p, None)),
        ('dt_replay_claim', (4, 0, 16, SEED, None, p, None)),
        ('dt_replay_claim', (4, 0, 16, SEED, p, None, None)),
        ('dt_stack_store', (p, -1, 3, order, None, p, 0, p, None)),
        ('dt_stack_store', (p, 4, 0, order, None, p, 0, p, None)),
        ('dt_stack_store', (p, 4, 3, None, None, p, 0, p, None)),
        ('dt_stack_store', (p, 4, 3, past, None, p, 0, p, None)),
        ('dt_stack_store', (p, 4, 3, below, None, p, 0, p, None)),
        ('dt_stack_store', (p, 4, 3, order, None, p, 2, p, None)),
        ('dt_stack_store', (None, 4, 3, order, None, p, 0, p, None)),
        ('dt_stack_store', (p, 4, 3, order, None, None, 0, p, None)),
        ('dt_stack_store', (p, 4, 3, order, None, p, 0, None, None)),
        ('dt_stack_store', (p, 4, 3, order, None, p, 0, q, None)),      # a misaligned store
        ('dt_stack_store', (q, 4, 3, order, None, p, 0, p, None)),
        ('dt_replay_commit', (-1, p, p, p, p, p, p, p, None)),
        ('dt_replay_draw', (-1, 0, 16, SEED, p, None)),
        ('dt_replay_draw', (4, -1, 16, SEED, p, None)),
        ('dt_replay_draw', (4, 0, 0, SEED, p, None)),
        ('dt_replay_draw', (4, 0, 2 ** 31, SEED, p, None)),
        ('dt_replay_draw', (4, 0, 16, SEED, None, None)),
        ('dt_cnn_replay_gather', (-1, p, p, p, p, p, 1, p, p, p, p, p, None)),
        ('dt_cnn_replay_gather', (32768, p, p, p, p, p, 1, p, p, p, p, p, None)),
        ('dt_cnn_replay_gather', (4, p, q, p, p, p, 1, p, p, p, p, p, None)),
        ('dt_cnn_replay_gather', (4, p, p, p, p, p, 0, q, p, p, p, p, None)),
        ('dt_cnn_replay_gather', (4, p, p, p, p, p, 1, p, q, p, p, p, None)),
    ]
    for k in range(1, 8):                       # each pointer of commit in turn
        a = [4] + [p] * 7 + [None]
        a[k] = None
        cases.append(('dt_replay_commit', tuple(a)))
    for k in (1, 2, 3, 4, 5, 7, 8, 9, 10, 11):  # each pointer of the gather
        a = [4, p, p, p, p, p, 1, p, p, p, p, p, None]
        a[k] = None
        cases.append(('dt_cnn_replay_gather', tuple(a)))
    for name, args in cases:
        assert getattr(L, name)(*args) == ARG, (name, args)
    # nothing to do is not an error
    assert L.dt_replay_claim(0, 0, 16, SEED, None, None, None) == 0
    assert L.dt_stack_store(None, 0, 3, order, None, None, 0, None, None) == 0
    assert L.dt_replay_commit(0, None, None, None, None, None, None, None, None) == 0
    assert L.dt_replay_draw(0, 0, 16, SEED, None, None) == 0
    assert L.dt_cnn_replay_gather(0, None, None, None, None, None, 1, None, None, None, None,
                                  None, None) == 0
    assert L.dt_abi_version() == 14             # new entry points only
    declared = _lib.exported_symbols()
    for name in {n for n, _ in cases}:
        assert name in declared, name
