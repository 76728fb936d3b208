"""The plain statement of `overlapnet_amd.infer.FeatureVolumeCache`, shared by tests/test_cache_growth_host.py (a fake engine on the
CPU) and tests/test_gpu_cache_growth.py (the real engine): a dict slot -> volume plus a high-water mark, a seeded generator of
operation sequences that walk the cache through its reallocations, the driver that applies a sequence to the model and to the real
class side by side, and the slot sequence one rank of a sharded `Infer` sees.

The model knows nothing about pools, capacities or copies: a slot holds the volume last written to it, `len()` is one past the highest
slot ever written, and a Delta row belongs to the head weights that were registered when the row was last (re)built.  The generator
does follow the allocation rule (`predicted_capacity`), only to AIM its operations at the reallocations; what a sequence really
reached is observed on the real class (`run_ops` logs the capacity around every operation) and asserted by the host test."""
import numpy as np
import torch

from overlapnet_amd import distributed as D

SEEDS = (11, 12, 13)          # the committed sequences (tests/test_cache_growth_host.py asserts what each of them reaches)
GROWTH_CAUSES = ("extend", "put_beyond", "put_slots", "append")


class CacheModel(object):
    def __init__(self):
        self.vols = {}            # slot -> (W, 128) volume, as the driver handed it in
        self.stamp = {}           # slot -> head version its Delta row was built under
        self.n = 0                # high-water mark: one past the highest slot ever written
        self.head_version = 0     # bumped by whoever re-registers the head; rows keep their stamp until `rebuild`

    def put(self, slot, vols):
        """k volumes at slot .. slot + k - 1: an overwrite below the end, an append at it, a write beyond it (the slots in between
        stay unwritten)."""
        for j, v in enumerate(vols):
            self.vols[slot + j] = v
            self.stamp[slot + j] = self.head_version
        self.n = max(self.n, slot + len(vols))

    def extend(self, vols):
        self.put(self.n, vols)

    def put_slots(self, slots, vols):
        assert len(slots) == len(vols) and len(set(slots)) == len(slots) and min(slots) >= 0
        for s, v in zip(slots, vols):
            self.put(int(s), [v])

    def append(self, vol):
        self.extend([vol])

    def rebuild(self):
        for s in self.vols:
            self.stamp[s] = self.head_version

    def slots(self):
        return sorted(self.vols)


def predicted_capacity(cap, need, min_capacity):
    """The allocation rule of `FeatureVolumeCache._grow`: exactly `need` (at least `min_capacity`) on first use, 2 x need afterwards."""
    if cap is not None and need <= cap:
        return cap
    return max(max(1, int(min_capacity)), need if cap is None else 2 * need)


def generate_ops(seed, min_capacity):
    """A list of operations: ('extend', ids) | ('put', slot, ids) | ('put_slots', slots, ids) | ('append', id) | ('rebuild',), `ids`
    naming fresh volumes 0, 1, 2, ... (the caller makes them).  After the first allocation each of GROWTH_CAUSES, in a seeded
    order, forces one reallocation; quiet operations (overwrites, appends that fit, scattered writes, rebuilds) stand in between,
    and an overwrite below the end follows every reallocation.  Returns (ops, number of volumes)."""
    rng = np.random.default_rng(seed)
    st = {"n": 0, "cap": None, "ids": 0}
    ops = []

    def ids(k):
        a = list(range(st["ids"], st["ids"] + int(k)))
        st["ids"] += int(k)
        return a

    def emit(op):
        ops.append(op)
        if op[0] == "extend":
            need = st["n"] + len(op[1])
        elif op[0] == "put":
            need = max(st["n"], op[1] + len(op[2]))
        elif op[0] == "put_slots":
            need = max(st["n"], max(op[1]) + 1)
        elif op[0] == "append":
            need = st["n"] + 1
        else:
            return
        st["cap"] = predicted_capacity(st["cap"], need, min_capacity)
        st["n"] = need

    def overwrite():
        k = int(rng.integers(1, 3)) if st["n"] >= 2 else 1
        return ("put", int(rng.integers(0, st["n"] - k + 1)), ids(k))

    def quiet():
        n, room = st["n"], st["cap"] - st["n"]
        kinds = ["overwrite", "scatter", "rebuild"] + (["append", "put_end", "extend"] if room >= 1 else [])
        kind = kinds[int(rng.integers(len(kinds)))]
        if kind == "overwrite":
            return overwrite()
        if kind == "scatter":
            m = int(rng.integers(1, min(3, n) + 1))
            return ("put_slots", [int(s) for s in rng.choice(n, size=m, replace=False)], ids(m))
        if kind == "append":
            return ("append", ids(1)[0])
        if kind == "put_end":
            return ("put", n, ids(1))
        if kind == "extend":
            return ("extend", ids(int(rng.integers(1, min(room, 3) + 1))))
        return ("rebuild",)

    def growing(cause):
        n, cap = st["n"], st["cap"]
        if cause == "extend":
            return [("extend", ids(cap - n + int(rng.integers(1, 3))))]
        if cause == "put_beyond":                      # strictly beyond the end: the slots in between stay unwritten
            return [("put", max(cap, n + 1) + int(rng.integers(0, 3)), ids(int(rng.integers(1, 3))))]
        if cause == "put_slots":                       # one slot past the capacity, the others overwrite; not in increasing order
            m = int(rng.integers(1, min(2, n) + 1))
            slots = [cap + int(rng.integers(0, 3))] + [int(s) for s in rng.choice(n, size=m, replace=False)]
            order = rng.permutation(len(slots))
            return [("put_slots", [slots[i] for i in order], ids(len(slots)))]
        fill = [("extend", ids(cap - n))] if cap > n else []         # 'append': fill the pools to the brim first
        return fill + [("append", ids(1)[0])]

    emit(("extend", ids(int(rng.integers(1, 3)))))                    # the first allocation
    for cause in rng.permutation(GROWTH_CAUSES):
        for _ in range(int(rng.integers(1, 4))):
            emit(quiet())
        for op in growing(str(cause)):
            emit(op)
        emit(overwrite())
    for _ in range(2):
        emit(quiet())
    emit(("rebuild",))
    return ops, st["ids"]


def capacity(cache):
    return None if cache._fv is None else int(cache._fv.shape[0])


def run_ops(cache, model, ops, vol, after=None, before_rebuild=None):
    """Apply `ops` to the real cache and to the model.  `vol(id)` -> the (W, 128) float32 tensor of volume `id` on the engine's device
    (the same object every time).  `before_rebuild()` runs ahead of every 'rebuild' (the host test re-registers its fake head there);
    `after(entry)` after every operation.  Returns the log: one dict per operation with its `kind` ('extend', 'put_below', 'put_end',
    'put_beyond', 'put_slots', 'append', 'rebuild'), the `slots` it wrote and the capacity and length around it."""
    log = []
    for i, op in enumerate(ops):
        entry = {"i": i, "op": op[0], "cap_before": capacity(cache), "n_before": len(cache), "slots": []}
        if op[0] == "extend":
            vs = [vol(j) for j in op[1]]
            entry.update(kind="extend", slots=list(range(model.n, model.n + len(vs))))
            cache.extend_device(torch.stack(vs))
            model.extend(vs)
        elif op[0] == "put":
            vs = [vol(j) for j in op[2]]
            kind = "put_below" if op[1] < model.n else ("put_end" if op[1] == model.n else "put_beyond")
            entry.update(kind=kind, slots=list(range(op[1], op[1] + len(vs))))
            cache.put_device(op[1], torch.stack(vs))
            model.put(op[1], vs)
        elif op[0] == "put_slots":
            vs = [vol(j) for j in op[2]]
            entry.update(kind="put_slots", slots=list(op[1]))
            cache.put_slots_device(op[1], torch.stack(vs))
            model.put_slots(op[1], vs)
        elif op[0] == "append":
            v = vol(op[1])
            entry.update(kind="append", slots=[model.n])
            cache.append(v.cpu().numpy().reshape((1,) + tuple(v.shape)))       # a host volume, as a caller of the reference's list would
            model.append(v)
        elif op[0] == "rebuild":
            entry.update(kind="rebuild")
            if before_rebuild is not None:
                before_rebuild()
            cache.rebuild_delta_cache()
            model.rebuild()
        else:
            raise ValueError(op)
        entry.update(cap_after=capacity(cache), n_after=len(cache))
        entry["grew"] = entry["cap_before"] is not None and entry["cap_after"] != entry["cap_before"]
        log.append(entry)
        if after is not None:
            after(entry)
    return log


def growth_causes(log):
    """kind of every operation that reallocated existing pools, in order."""
    return [e["kind"] for e in log if e["grew"]]


def overwrites_after_growth(log):
    """Operations that overwrote below the end after some reallocation had happened."""
    seen, out = False, []
    for e in log:
        if seen and e["kind"] == "put_below":
            out.append(e)
        seen = seen or e["grew"]
    return out


def landmark_slots(log, model):
    """Slots a sweep over the grown cache should sample: per reallocation the last slot written before it and the first written by
    the operation that caused it, and the slots written more than once -> (before, after, overwritten), each a sorted list of slots
    the model holds."""
    before, after, count = set(), set(), {}
    last = None
    for e in log:
        if e["grew"]:
            if last is not None:
                before.add(last)
            after.add(e["slots"][0])
        for s in e["slots"]:
            count[s] = count.get(s, 0) + 1
        if e["slots"]:
            last = e["slots"][-1]
    held = set(model.vols)
    return sorted(before & held), sorted(after & held), sorted(s for s, c in count.items() if c > 1 and s in held)


def sharded_slots(n_frames, rank, world):
    """[(frame id, local slot)] of the frames 0 .. n_frames - 1 that `rank` of `world` keeps, in the order they are fed: what
    `Infer._query_frame_sharded` hands to `put_device` on that rank (no process group involved)."""
    return [(f, int(D.frame_slot(f, world))) for f in range(int(n_frames)) if int(D.frame_owner(f, world)) == int(rank)]
