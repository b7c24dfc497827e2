"""TEST INFRASTRUCTURE ONLY -- the CPU restatement of aido1_amd.cnn_replay's
slot rules (include/dtreplay.h dt_replay_claim / dt_replay_draw) in plain
Python integers, on the oracle's Philox (oracle/philox_ref.py).

duckietown_rl/utils.py:18-57 pops a uniformly drawn list position from a full
buffer and appends; it samples list positions uniformly.  In slot form:
transition s (the count of every add) takes slot s while s < max_size, else
the slot its own Philox block draws; a draw d (the count of every draw) reads
the slot its block draws among the len filled ones."""
from oracle.philox_ref import key_of, philox4x32_10

TAG_EVICT = 0x45564943      # 'EVIC'
TAG_SAMPLE = 0x534D504C     # 'SMPL'


def _pick(serial, tag, rng, seed):
    w = philox4x32_10((serial & 0xFFFFFFFF, serial >> 32, 0, tag), key_of(seed))[0]
    return (w * rng) >> 32


def slot_of(s, max_size, seed):
    return s if s < max_size else _pick(s, TAG_EVICT, max_size, seed)


def slots_of(added, n, max_size, seed):
    """The slot of each of the n adds that follow `added` earlier ones."""
    return [slot_of(added + i, max_size, seed) for i in range(n)]


def rows_of(added, n, max_size, seed):
    """slots_of, with -1 for an add that a later add of the same batch
    evicts (the higher serial keeps the slot)."""
    slots = slots_of(added, n, max_size, seed)
    last = {sl: i for i, sl in enumerate(slots)}
    return [sl if last[sl] == i else -1 for i, sl in enumerate(slots)]


def draws_of(drawn, batch, length, seed):
    """The slots of draws drawn .. drawn + batch - 1 over `length` filled slots."""
    return [_pick(drawn + i, TAG_SAMPLE, length, seed) for i in range(batch)]


def serials_after(batches, max_size, seed):
    """storage_serials() after the batches, from added = 0: each slot's
    serial, -1 where never written."""
    held, added = [-1] * max_size, 0
    for n in batches:
        for i, row in enumerate(rows_of(added, n, max_size, seed)):
            if row >= 0:
                held[row] = added + i
        added += n
    return held
