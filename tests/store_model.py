"""The store as a dictionary, and seeded write histories for it: TEST
INFRASTRUCTURE, the expectation of tests/test_store.py for the whole chain
(wal_recover_table, memtable_from_batches, db_scan, sst_get_values,
sst_compact_tables) and of tests/test_store_model.py for the composition of
the per-stage models.

The model knows nothing of internal keys, trailers, runs or tables: a reader
at sequence s sees, of every user key, its last write at or before s. It is
not pinned to the reference because it needs none: it is the statement the
reference's format exists to provide.
"""
from __future__ import annotations

import functools
from typing import List, Optional, Sequence, Tuple

import numpy as np

import log_synth
import memtable_model as mm

Op = Tuple[int, bytes, Optional[bytes]]  # sequence, user key, value (None: a deletion)


class Store:
    """A list of operations and what a reader at a snapshot sees of it."""

    def __init__(self, ops: Sequence[Op] = ()):
        self.ops: List[Op] = list(ops)
        self.of = {}  # user key -> its operations
        for op in self.ops:
            self.of.setdefault(op[1], []).append(op)

    def last(self, user: bytes, snapshot: int) -> Optional[Op]:
        """The operation on `user` with the highest sequence at or below
        `snapshot`, None for none."""
        seen = [op for op in self.of.get(user, ()) if op[0] <= snapshot]
        return max(seen, key=lambda op: op[0]) if seen else None

    def get(self, user: bytes, snapshot: int) -> Optional[bytes]:
        """The value a reader at `snapshot` sees, None for "absent"."""
        op = self.last(user, snapshot)
        return None if op is None else op[2]

    def scan(self, start: bytes, limit: Optional[bytes], snapshot: int,
             max_count: Optional[int] = None, reverse: bool = False):
        """[(user key, value)] of the keys in [start, limit) a reader at
        `snapshot` sees, in bytes order, the first max_count of them; with
        reverse those same entries last first."""
        users = sorted(u for u in self.of if u >= start and (limit is None or u < limit))
        seen = [(u, self.get(u, snapshot)) for u in users]
        seen = [(u, v) for u, v in seen if v is not None][:max_count]
        return seen[::-1] if reverse else seen


# ---- the keys -------------------------------------------------------------------------------

STEM = b"shared-prefix-of-pairs"  # 22 bytes
LONG = bytes(range(33, 33 + 200)) + b"long-key-stem" * 7 + b"12345678"  # 299 bytes
ZEROS = [b"", b"\x00", b"\x00\x00", b"a", b"a\x00", b"a\x00\x00"]
ONES = [b"\xff" * 7, b"\xff" * 8, b"\xff" * 9, b"\xff" * 8 + b"\x00"]
PAIR_AT = (8, 9, 15, 16, 17)
PAIRS = [STEM[:at] + bytes([x]) + STEM[at + 1:] for at in PAIR_AT for x in (0x7f, 0x80)]
LONGS = [LONG + b"\x01", LONG + b"\x02"]
SPECIAL = ZEROS + ONES + PAIRS + LONGS
EVERY_GROUP = b"\xff" * 8        # rewritten in every group
DELETED_LAST = b"a\x00"          # deleted at the top sequence
ONLY_OLDEST, ONLY_NEWEST = b"only-in-the-oldest-group", b"only-in-the-memtable"
# absent keys. Nothing sorts below the first key, b"": the key just below the first
# non-empty one of its family stands for it. Then between and around the special keys'
# near misses, just above the last key, and ten 0xff bytes.
ABSENT = [b"\x00\x00\x00", b"\x00\x01", b"`", b"a\x00\x00\x00", b"a\x01", b"\xff" * 6,
          b"\xff" * 8 + b"\x01", b"\xff" * 9 + b"\x00", b"\xff" * 10,
          STEM[:8] + b"\x7e" + STEM[9:], STEM[:8] + b"\x81" + STEM[9:], STEM[:17], STEM,
          LONG, LONG + b"\x03", b"only-in"]

KV_SEP = (16, 64, 16, 64)  # a group's threshold (the last: the memtable's, when it is flushed)
# a seed's groups: each has one of more than a sort tile (1024), the second more than a scan
# tile (4096) in all
SIZES = ((1100, 320, 400, 350), (1150, 1050, 1100, 1000), (340, 310, 450, 1040))
SEEDS = tuple(range(len(SIZES)))


class History:
    """What history(seed) returns: groups[g] the write batches of group g,
    ops[g] the same writes as the model's operations; the last group is the
    live memtable, the others become level-0 tables (oldest first)."""

    def __init__(self, seed, groups, ops, users):
        self.seed, self.groups, self.ops, self.users = seed, groups, ops, users
        self.file_numbers = [11 + 3 * g + seed for g in range(len(groups))]
        self.kv_sep = KV_SEP[:len(groups)]
        self.block_size, self.restart_interval = (256, 384, 512)[seed % 3], 4
        self.first = [o[0][0] for o in ops]
        self.last = [o[-1][0] for o in ops]

    def store(self, groups=None) -> Store:
        return Store([op for g in (range(len(self.ops)) if groups is None else groups)
                      for op in self.ops[g]])

    def payload(self, g: int):
        """(payload, batch offsets, batch lengths) of group g, end to end."""
        offs, at = [], 0
        for b in self.groups[g]:
            offs.append(at)
            at += len(b)
        return b"".join(self.groups[g]), offs, [len(b) for b in self.groups[g]]

    def log(self, g: int) -> bytes:
        """Group g framed as the reference's WAL, a batch a record."""
        w = log_synth.LogWriter()
        for b in self.groups[g]:
            w.add_record(b)
        return bytes(w.buf)

    def snapshots(self) -> List[int]:
        """0, below the first write, the last sequence of each group, one
        strictly inside each group, the top, kMaxSequenceNumber."""
        inside = [(a + b) // 2 for a, b in zip(self.first, self.last)]
        return sorted({0, self.first[0] - 1, *self.last, *inside, (1 << 56) - 1})

    def ranges(self):
        """(start, limit, max_count) of one db_scan call."""
        users = self.users
        out = [(b"", None, None)]
        out += [(k, k + b"\x00", 1) for k in users + ABSENT]
        mid, late = users[len(users) // 3], users[2 * len(users) // 3]
        out += [(mid, mid, None), (late, mid, None), (mid, None, 0), (mid, late, None),
                (b"", late, 7), (ONES[0], None, None)]
        return out


@functools.lru_cache(maxsize=None)
def history(seed: int) -> History:
    rng = np.random.default_rng(7000 + seed)
    ordinary = sorted({rng.integers(97, 123, int(rng.integers(1, 25)), dtype=np.uint8).tobytes()
                       for _ in range(36)} - set(SPECIAL))
    users = sorted(set(SPECIAL + ordinary + [ONLY_OLDEST, ONLY_NEWEST]))
    assert not set(ABSENT) & set(users)
    sizes = SIZES[seed % len(SIZES)]
    ngroups = len(sizes)
    groups, ops, seq = [], [], 100 + 1000 * seed
    for g, size in enumerate(sizes):
        here = [u for u in users if (u != ONLY_OLDEST or g == 0) and
                (u != ONLY_NEWEST or g == ngroups - 1)]
        # every key of the group once, in a seeded order, then seeded picks
        picks = [here[i] for i in rng.permutation(len(here))]
        picks += [here[int(i)] for i in rng.integers(0, len(here), size - len(picks))]
        written, batches, gops = set(), [], []
        at = 0
        while at < size:
            # (the first batch is longer than the parse window of 8192 bytes)
            count = min(size - at, 220 if at == 0 else int(rng.integers(1, 60)))
            body = b""
            for j in range(count):
                user = picks[at + j]
                top = g == ngroups - 1 and at + j == size - 1
                if top:
                    user = DELETED_LAST
                first = user not in written
                written.add(user)
                deletes = top or (not first and rng.random() < 0.2) or \
                    (first and g > 0 and user not in (EVERY_GROUP, ONLY_NEWEST) and rng.random() < 0.1)
                if deletes:
                    body += mm.delete(user)
                    gops.append((seq + at + j, user, None))
                else:
                    v = rng.integers(0, 256, int(rng.integers(0, 81)), dtype=np.uint8).tobytes()
                    body += mm.put(user, b"\x02" + v)  # EncodeNonIndexValue
                    gops.append((seq + at + j, user, v))
            batches.append(mm.batch(seq + at, count, body))
            at += count
        seq += size
        groups.append(batches)
        ops.append(gops)
    return History(seed, groups, ops, users)
