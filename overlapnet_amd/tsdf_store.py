"""What leaves the rolling TSDF window is kept, and put back when the window returns (ovn_tsdf_window_brick_flags / _page_out /
_page_in, include/ovn_hip_tsdf_store.h, csrc/tsdf_store.hip).

    vol = RollingTsdfVolume(engine, extent=(120, 120, 24), voxel=0.2, store=True)
    vol.follow(position); vol.integrate(...)           # bricks that leave go to vol.store, bricks that return come back
    mesh = vol.mesh()                                  # every cell of window and store, once
    vol.store.save("map.npz"); store = TsdfBrickStore.load(engine, "map.npz")

A window's dimensions, base and shifts are multiples of 8, so what leaves and what enters is a whole number of aligned 8 x 8 x 8
lattice BRICKS; brick (bi, bj, bk) holds the samples 8 bi .. 8 bi + 7 on x and likewise on y and z.  `TsdfBrickStore` keeps the bricks
that differ from fresh storage in a device pool of 4 KB slots, with the index (brick -> slot) and the free list on the host.  A brick
lives in the store or in the window, never in both.  Nothing here is on by default: without `store=` a RollingTsdfVolume makes the
launches it always made.
"""
from __future__ import annotations

import heapq
import zipfile
from types import SimpleNamespace
from typing import Dict, List, Sequence, Tuple

import numpy as np

from ._lib import OvnError

BRICK = 8
BRICK_WORDS = 1024               # OVN_TSDF_BRICK_WORDS: 512 tsdf words, then 512 weight words
BRICK_BYTES = 4 * BRICK_WORDS
Key = Tuple[int, int, int]


# ---- the three native calls -------------------------------------------------------------------------------------------------------------
def _window_args(engine, what: str, tsdf, weight, base):
    engine._check(tsdf, "%s: tsdf (nz,ny,nx)" % what, ndim=3)
    engine._check(weight, "%s: weight (nz,ny,nx)" % what, shape=tuple(tsdf.shape))
    nz, ny, nx = (int(v) for v in tsdf.shape)
    return nx, ny, nz, engine._int3(what, "base", base)


def window_brick_flags(engine, tsdf, weight, base, box_lo, box_hi, out=None):
    """(hi - lo)[::-1] uint8 device tensor, z-major: 1 for every brick of the box box_lo .. box_hi (lattice BRICK coordinates, hi
    exclusive, inside the window at `base`) with a sample whose words differ from (tsdf 1.0, weight 0.0) (ovn_tsdf_window_brick_flags).
    out: a contiguous uint8 tensor of that many elements to write into."""
    import torch
    from .engine import _ptr
    what = "window_brick_flags"
    nx, ny, nz, b3 = _window_args(engine, what, tsdf, weight, base)
    lo3, hi3 = engine._int3(what, "box_lo", box_lo), engine._int3(what, "box_hi", box_hi)
    count = tuple(int(h) - int(l) for l, h in zip(lo3, hi3))
    if any(c < 0 for c in count):
        raise OvnError("%s: box %s .. %s has lo > hi" % (what, list(lo3), list(hi3)))
    if out is None:
        out = torch.empty(count[::-1], dtype=torch.uint8, device=engine.device)
    else:
        engine._check(out, "%s: out" % what, torch.uint8, numel=count[0] * count[1] * count[2])
    engine._call("ovn_tsdf_window_brick_flags", engine._stream(), _ptr(tsdf), _ptr(weight), nx, ny, nz, b3, lo3, hi3, _ptr(out))
    return out


def _page(engine, name: str, tsdf, weight, base, bricks, slots, pool) -> None:
    import torch
    from .engine import _ptr
    nx, ny, nz, b3 = _window_args(engine, name, tsdf, weight, base)
    engine._check(bricks, "%s: bricks (n,3)" % name, torch.int32, ndim=2)
    n = int(bricks.shape[0])
    if int(bricks.shape[1]) != 3:
        raise OvnError("%s: bricks must be (n,3), got %s" % (name, tuple(bricks.shape)))
    engine._check(slots, "%s: slots (n)" % name, torch.int32, (n,))
    engine._check(pool, "%s: pool" % name, ndim=1)
    if pool.numel() % BRICK_WORDS:
        raise OvnError("%s: the pool must hold %d words per slot, got %d words" % (name, BRICK_WORDS, pool.numel()))
    engine._call("ovn_tsdf_" + name, engine._stream(), _ptr(tsdf), _ptr(weight), nx, ny, nz, b3, n, _ptr(bricks), _ptr(slots), _ptr(pool))


def window_page_out(engine, tsdf, weight, base, bricks, slots, pool) -> None:
    """Each brick of `bricks` ((n,3) int32 device tensor of lattice brick coordinates inside the window) copied from the ring into
    slot `slots[i]` ((n) int32) of `pool` (float32, 1024 words per slot) (ovn_tsdf_window_page_out).  The window is not written."""
    _page(engine, "window_page_out", tsdf, weight, base, bricks, slots, pool)


def window_page_in(engine, tsdf, weight, base, bricks, slots, pool) -> None:
    """The reverse of `window_page_out`: pool slot -> ring (ovn_tsdf_window_page_in).  The pool is not written."""
    _page(engine, "window_page_in", tsdf, weight, base, bricks, slots, pool)


# ---- boxes, bricks and the tiles of the mesh sweep -----------------------------------------------------------------------------------
def brick_box(lo, hi):
    """The sample box lo .. hi (hi exclusive, multiples of 8) in brick coordinates."""
    lo, hi = [int(v) for v in lo], [int(v) for v in hi]
    if any(v % BRICK for v in lo + hi):
        raise ValueError("a box of whole bricks has corners that are multiples of 8, got %s .. %s" % (lo, hi))
    return tuple(v // BRICK for v in lo), tuple(v // BRICK for v in hi)


def _zyx(key: Key):
    return key[2], key[1], key[0]


def sweep_tiles(keys: Sequence[Key], shape) -> List[Tuple[Key, Key, Key, List[Key]]]:
    """The tiles of the mesh sweep over the bricks `keys` for a window of `shape` samples: [(base, cell_lo, cell_hi, keys of the tile)].

    With lo = 8 min(keys) per axis, tile (a, b, c) holds the samples base = lo + (a, b, c) (n - 8) .. base + n - 1 and OWNS the cells
    whose low corner lies in cell_lo = base .. cell_hi = base + n - 8 (exclusive): tiles overlap by one brick, so the far corners of a
    tile's own cells are its own samples, and the own boxes partition the lattice from lo on.  Only tiles that hold a brick are listed
    (a tile without one has no surface), in ascending (z, y, x) order, each with its bricks in ascending (z, y, x) order."""
    n = [int(v) for v in shape]
    if not keys:
        return []
    k = np.asarray(sorted(set(keys)), np.int64).reshape(-1, 3)
    lo = k.min(axis=0) * BRICK
    step = np.asarray(n, np.int64) - BRICK
    first = k * BRICK - lo                                   # the brick's first sample, from lo
    hi_tile = first // step                                  # the last tile that holds it ...
    lo_tile = np.maximum(hi_tile - (first % step == 0), 0)   # ... and the one before, whose last brick it is
    tiles: Dict[Key, List[Key]] = {}
    for key, t0, t1 in zip(map(tuple, k.tolist()), lo_tile.tolist(), hi_tile.tolist()):
        for c in range(t0[2], t1[2] + 1):
            for b in range(t0[1], t1[1] + 1):
                for a in range(t0[0], t1[0] + 1):
                    tiles.setdefault((a, b, c), []).append(key)
    out = []
    for t in sorted(tiles, key=_zyx):
        base = tuple(int(lo[a] + t[a] * step[a]) for a in range(3))
        out.append((base, base, tuple(int(base[a] + step[a]) for a in range(3)), sorted(tiles[t], key=_zyx)))
    return out


# ---- the store ------------------------------------------------------------------------------------------------------------------------
class TsdfBrickStore(object):
    """The bricks that left a rolling window: a device pool of 4 KB slots that grows by doubling, a host dict brick -> slot and a free
    list.  `max_bytes` caps the pool: a page-out that would pass it raises OvnError before anything is written.  There is no spill to
    host memory or disk.  A shift moves two small lists host to device and one flag array device to host."""

    def __init__(self, engine, max_bytes: int = 4 << 30):
        if int(max_bytes) < BRICK_BYTES:
            raise ValueError("max_bytes must hold at least one brick of %d bytes, got %r" % (BRICK_BYTES, max_bytes))
        self.engine = engine
        self.max_bytes = int(max_bytes)
        self._index: Dict[Key, int] = {}
        self._free: List[int] = []           # a heap: the lowest free slot is taken first
        self._top = 0                        # slots 0 .. _top - 1 are in the index or in the free list
        self._pool = None                    # float32 (capacity * 1024,), on the engine's device
        self.meta = None                     # dict(voxel, anchor, trunc, max_weight) of the volume the bricks belong to

    # -- accessors
    def __len__(self) -> int:
        return len(self._index)

    @property
    def bytes(self) -> int:
        """The bytes of the bricks held (the pool may be larger)."""
        return len(self._index) * BRICK_BYTES

    @property
    def capacity(self) -> int:
        return 0 if self._pool is None else self._pool.numel() // BRICK_WORDS

    def bricks(self) -> List[Key]:
        return sorted(self._index)

    def __contains__(self, key) -> bool:
        return tuple(int(v) for v in key) in self._index

    def get(self, key):
        """(tsdf, weight), two (8,8,8) float32 host arrays indexed [z, y, x], of a stored brick; KeyError for one not held."""
        slot = self._index[tuple(int(v) for v in key)]
        words = self._pool[slot * BRICK_WORDS:(slot + 1) * BRICK_WORDS].cpu().numpy()
        return words[:512].reshape(8, 8, 8).copy(), words[512:].reshape(8, 8, 8).copy()

    def clear(self) -> None:
        """Forgets every brick; the pool's memory is kept."""
        self._index, self._free, self._top = {}, [], 0

    def bind(self, volume) -> None:
        """Ties the store to the lattice of `volume`: an empty store without a lattice takes it, any other must agree in voxel,
        anchor and trunc (a loaded map continues only on the lattice it was built on)."""
        meta = dict(voxel=float(volume.voxel), anchor=np.asarray(volume.origin, np.float64).copy(), trunc=float(volume.trunc),
                    max_weight=float(volume.max_weight))
        if self.meta is None:
            self.meta = meta
            return
        for k in ("voxel", "anchor", "trunc"):
            if not np.array_equal(np.asarray(self.meta[k]), np.asarray(meta[k])):
                raise ValueError("the store holds bricks of a lattice with %s %s, the volume has %s" % (k, self.meta[k], meta[k]))

    # -- the pool
    def _reserve(self, n_new: int) -> None:
        """Room for n_new more bricks, or OvnError with nothing changed."""
        beyond = max(0, n_new - len(self._free))
        need = self._top + beyond
        if need * BRICK_BYTES > self.max_bytes:
            raise OvnError("TsdfBrickStore: %d bricks leave the window and %d are held: %d slots of %d bytes pass max_bytes = %d "
                           "(nothing was written; host spill is not supported)" % (n_new, len(self._index), need, BRICK_BYTES, self.max_bytes))
        if need > self.capacity:
            import torch
            cap = min(max(need, 2 * self.capacity, 64), max(self.max_bytes // BRICK_BYTES, need))
            pool = torch.empty(cap * BRICK_WORDS, dtype=torch.float32, device=self.engine.device)
            if self._pool is not None and self._top:
                pool[:self._top * BRICK_WORDS].copy_(self._pool[:self._top * BRICK_WORDS])
            self._pool = pool

    def _lists(self, keys: Sequence[Key], slots: Sequence[int]):
        import torch
        dev = self.engine.device
        return (torch.from_numpy(np.asarray(keys, np.int32).reshape(-1, 3)).to(dev), torch.from_numpy(np.asarray(slots, np.int32)).to(dev))

    # -- paging
    def page_out(self, volume, boxes) -> int:
        """Copies the non-empty bricks of the sample boxes [(lo, hi)] (hi exclusive; `leaving_boxes(old, new, shape)`) of the window
        `volume` (its tsdf, weight, shape and base) into the store -> how many.  The window is not written: the shift that follows
        clears the slots.  One flag array comes back from the device; the bricks are listed in ascending (z, y, x) order and take the
        free slots in ascending order, then new ones."""
        import torch
        bb = [brick_box(lo, hi) for lo, hi in boxes]
        counts = [int(np.prod([h - l for l, h in zip(lo, hi)])) for lo, hi in bb]
        if sum(counts) == 0:
            return 0
        flags = torch.empty(sum(counts), dtype=torch.uint8, device=self.engine.device)
        at = 0
        for (lo, hi), c in zip(bb, counts):
            if c:
                window_brick_flags(self.engine, volume.tsdf, volume.weight, volume.base, lo, hi, out=flags[at:at + c])
            at += c
        host = flags.cpu().numpy()                                                 # the one read-back
        keys, at = [], 0
        for (lo, hi), c in zip(bb, counts):
            f = host[at:at + c].reshape(hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0])
            z, y, x = np.nonzero(f)
            keys += list(zip((x + lo[0]).tolist(), (y + lo[1]).tolist(), (z + lo[2]).tolist()))
            at += c
        keys.sort(key=_zyx)
        if not keys:
            return 0
        held = [k for k in keys if k in self._index]
        if held:
            raise OvnError("TsdfBrickStore: brick %s is in the window and in the store" % (held[0],))
        self._reserve(len(keys))
        slots = []
        for _ in keys:
            if self._free:
                slots.append(heapq.heappop(self._free))
            else:
                slots.append(self._top)
                self._top += 1
        d_keys, d_slots = self._lists(keys, slots)
        window_page_out(self.engine, volume.tsdf, volume.weight, volume.base, d_keys, d_slots, self._pool)
        self._index.update(zip(keys, slots))
        return len(keys)

    def _held_in(self, boxes) -> List[Key]:
        """The stored bricks inside the sample boxes, ascending (z, y, x)."""
        bb = [brick_box(lo, hi) for lo, hi in boxes]
        cells = sum(int(np.prod([h - l for l, h in zip(lo, hi)])) for lo, hi in bb)
        inside = lambda k: any(all(l <= v < h for v, l, h in zip(k, lo, hi)) for lo, hi in bb)
        if cells > len(self._index):
            found = [k for k in self._index if inside(k)]
        else:
            found = [(x, y, z) for lo, hi in bb for z in range(lo[2], hi[2]) for y in range(lo[1], hi[1]) for x in range(lo[0], hi[0])
                     if (x, y, z) in self._index]
        return sorted(found, key=_zyx)

    def _copy_in(self, volume, keys: List[Key]) -> List[int]:
        slots = [self._index[k] for k in keys]
        if keys:
            d_keys, d_slots = self._lists(keys, slots)
            window_page_in(self.engine, volume.tsdf, volume.weight, volume.base, d_keys, d_slots, self._pool)
        return slots

    def page_in(self, volume, boxes) -> int:
        """Copies the stored bricks of the sample boxes [(lo, hi)] (`leaving_boxes(new, old, shape)`: what entered) into the window
        `volume` and frees their slots -> how many."""
        keys = self._held_in(boxes)
        for k, s in zip(keys, self._copy_in(volume, keys)):
            del self._index[k]
            heapq.heappush(self._free, s)
        return len(keys)

    # -- a file
    def _payload(self):
        keys = self.bricks()
        if not keys:
            return np.zeros((0, 3), np.int32), np.zeros((0, BRICK_WORDS), np.float32)
        import torch
        rows = torch.from_numpy(np.asarray([self._index[k] for k in keys], np.int64)).to(self.engine.device)
        pool = self._pool[:self._top * BRICK_WORDS].view(self._top, BRICK_WORDS)
        return np.asarray(keys, np.int32), pool.index_select(0, rows).cpu().numpy()

    def save(self, path: str, window=None) -> int:
        """One .npz: keys (n,3) int32 in sorted order, payload (n,1024) float32, voxel, anchor, trunc, max_weight -> n.  The archive's
        entries carry a fixed date, so stores of equal content are equal files.  window: the RollingTsdfVolume whose store this is --
        its non-empty bricks are written too (copies: window and store stay as they are), so the file is the whole map."""
        if self.meta is None:
            raise OvnError("TsdfBrickStore.save: the store belongs to no volume yet (no voxel, anchor or trunc to write)")
        keys, payload = self._payload()
        if window is not None:
            live = TsdfBrickStore(self.engine, max_bytes=max(BRICK_BYTES, int(np.prod(window.shape)) * 8))
            live.page_out(window, [(tuple(window.base), tuple(b + n for b, n in zip(window.base, window.shape)))])
            more, words = live._payload()
            keys, payload = np.concatenate([keys, more]), np.concatenate([payload, words])
            order = sorted(range(keys.shape[0]), key=lambda i: tuple(keys[i].tolist()))
            keys, payload = np.ascontiguousarray(keys[order]), np.ascontiguousarray(payload[order])
        entries = [("keys", keys), ("payload", payload), ("voxel", np.float64(self.meta["voxel"])),
                   ("anchor", np.asarray(self.meta["anchor"], np.float64)), ("trunc", np.float64(self.meta["trunc"])),
                   ("max_weight", np.float64(self.meta["max_weight"]))]
        with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED, allowZip64=True) as z:
            for name, a in entries:
                info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
                with z.open(info, "w", force_zip64=True) as f:
                    np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)
        return int(keys.shape[0])

    @classmethod
    def load(cls, engine, path: str, max_bytes: int = 4 << 30) -> "TsdfBrickStore":
        """The store `save` wrote: brick i of the sorted keys in slot i."""
        import torch
        with np.load(path, allow_pickle=False) as z:
            keys, payload = np.asarray(z["keys"]), np.asarray(z["payload"])
            meta = dict(voxel=float(z["voxel"]), anchor=np.asarray(z["anchor"], np.float64).reshape(3), trunc=float(z["trunc"]),
                        max_weight=float(z["max_weight"]))
        n = int(keys.shape[0])
        if keys.shape != (n, 3) or keys.dtype != np.int32 or payload.shape != (n, BRICK_WORDS) or payload.dtype != np.float32:
            raise OvnError("%s: keys %s %s and payload %s %s are not (n,3) int32 and (n,1024) float32"
                           % (path, keys.shape, keys.dtype, payload.shape, payload.dtype))
        store = cls(engine, max_bytes=max_bytes)
        store.meta = meta
        if n:
            store._reserve(n)
            store._pool[:n * BRICK_WORDS].copy_(torch.from_numpy(np.ascontiguousarray(payload).reshape(-1)).to(engine.device))
            store._index = {tuple(int(v) for v in k): i for i, k in enumerate(keys.tolist())}
            if len(store._index) != n:
                raise OvnError("%s: a brick is listed twice" % path)
            store._top = n
        return store

    # -- the mesh of window and store
    def triangles(self, volume, min_weight: float = 1.0):
        """(T,3,3) float32 device tensor: the triangles of every cell of the store's bricks and the window's, each cell once.  The
        bounding box of all bricks is swept in tiles of the window's shape that step by n - 8 (`sweep_tiles`); a tile's bricks are
        copied into a scratch volume of the window's shape and its own cells extracted with ovn_tsdf_window_triangles.  The window's
        bricks come from a temporary store (a copy); window, base and store are not written."""
        import torch
        eng = self.engine
        shape = tuple(volume.shape)
        whole = [(tuple(volume.base), tuple(b + n for b, n in zip(volume.base, shape)))]
        live = TsdfBrickStore(eng, max_bytes=max(BRICK_BYTES, int(np.prod(shape)) * 8))
        live.page_out(volume, whole)
        tiles = sweep_tiles(list(self._index) + list(live._index), shape)
        scratch = SimpleNamespace(tsdf=torch.empty_like(volume.tsdf), weight=torch.empty_like(volume.weight), base=None)
        parts = []
        for base, lo, hi, keys in tiles:
            scratch.base = base
            scratch.tsdf.fill_(1.0)
            scratch.weight.zero_()
            for store in (self, live):               # a brick has one home: the two lists are disjoint
                store._copy_in(scratch, [k for k in keys if k in store._index])
            tri, total = eng.tsdf_triangles(scratch.tsdf, scratch.weight, volume.origin, volume.voxel, min_weight, base=base, box=(lo, hi))
            if total:
                parts.append(tri)
        if not parts:
            return torch.zeros((0, 3, 3), dtype=torch.float32, device=eng.device)
        return torch.cat(parts)


def mesh_from_store(store: TsdfBrickStore, shape=(128, 128, 64), min_weight: float = 1.0):
    """The TriangleMesh of a store alone (a saved map, `tools/build_mesh.py --load-volume`): the sweep of `TsdfBrickStore.triangles`
    through an empty window of `shape` samples on the store's lattice."""
    from .tsdf import RollingTsdfVolume
    if store.meta is None:
        raise OvnError("mesh_from_store: the store belongs to no volume (no voxel or anchor)")
    m = store.meta
    vol = RollingTsdfVolume(store.engine, tuple(n * m["voxel"] for n in shape), m["voxel"], trunc=m["trunc"], max_weight=m["max_weight"],
                            anchor=m["anchor"], store=store)
    return vol.mesh(min_weight)
