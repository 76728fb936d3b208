"""NumPy model of the brick store behind the rolling TSDF window (include/ovn_hip_tsdf_store.h, overlapnet_amd/tsdf_store.py;
DESIGN.md section 38): a dict of 8 x 8 x 8 blocks around `_tsdf_window_ref.shift`.

`Model` is the statement: a window in ring storage plus `store`, a dict brick -> (tsdf, weight) blocks indexed [z, y, x].  Moving the
window keeps every brick that leaves with a word different from fresh storage, clears the slots that change hands, and puts back the
kept bricks that enter.  It works on whatever bits it is given, so next to the GPU it is fed the GPU's own window.  `World` is the
thing both must equal: a dict of samples that never forgets.  `HostLib` stands in for the CDLL on CPU tensors -- the three store calls
and ovn_tsdf_window_shift, each by its statement -- so that `TsdfBrickStore` and `RollingTsdfVolume(store=...)` run without a GPU.
"""
import ctypes as C

import numpy as np

import _tsdf_window_ref as WR

F32 = np.float32
ONE_BITS = np.uint32(0x3f800000)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def window_bricks(base, shape):
    """The bricks (bi, bj, bk) of the window `shape` at `base`, ascending (z, y, x)."""
    r = [range(b // 8, (b + n) // 8) for b, n in zip(base, shape)]
    return [(x, y, z) for z in r[2] for y in r[1] for x in r[0]]


def brick_differs(t, w):
    """Whether a brick holds a word that is not fresh storage's: the comparison is of bit patterns."""
    return bool((bits(t) != ONE_BITS).any() or (bits(w) != 0).any())


def _brick_index(key, dims):
    """np.ix_ of a brick's slots in ring storage (nz,ny,nx)."""
    nz, ny, nx = dims
    s = [WR.slots_of(np.arange(8 * k, 8 * k + 8), n) for k, n in zip(key, (nx, ny, nz))]
    return np.ix_(s[2], s[1], s[0])


class Model(object):
    def __init__(self, shape, base, tsdf=None, weight=None):
        self.shape, self.base = tuple(shape), tuple(base)
        nx, ny, nz = self.shape
        self.tsdf = np.ones((nz, ny, nx), F32) if tsdf is None else np.array(tsdf, F32)
        self.weight = np.zeros((nz, ny, nx), F32) if weight is None else np.array(weight, F32)
        self.store = {}

    def move(self, new_base):
        new_base = tuple(int(v) for v in new_base)
        old = set(window_bricks(self.base, self.shape))
        new = set(window_bricks(new_base, self.shape))
        for key in sorted(old - new):
            ix = _brick_index(key, self.tsdf.shape)
            t, w = self.tsdf[ix].copy(), self.weight[ix].copy()
            if brick_differs(t, w):
                assert key not in self.store, "a brick with two homes"
                self.store[key] = (t, w)
        self.tsdf, self.weight, _ = WR.shift(self.tsdf, self.weight, self.base, new_base)
        self.base = new_base
        for key in sorted(new - old):
            if key in self.store:
                ix = _brick_index(key, self.tsdf.shape)
                self.tsdf[ix], self.weight[ix] = self.store.pop(key)

    def write(self, index, t, w):
        """One sample at lattice `index` (inside the window)."""
        s = tuple(int(WR.slots_of(i, n)) for i, n in zip(index, self.shape))
        assert all(b <= i < b + n for i, b, n in zip(index, self.base, self.shape))
        self.tsdf[s[2], s[1], s[0]], self.weight[s[2], s[1], s[0]] = F32(t), F32(w)


class World(object):
    """Every sample ever written, by lattice index -> (tsdf bits, weight bits); what was never written is fresh."""

    def __init__(self):
        self.samples = {}

    def write(self, index, t, w):
        self.samples[tuple(int(v) for v in index)] = (int(bits(F32(t)).reshape(-1)[0]), int(bits(F32(w)).reshape(-1)[0]))

    def block(self, lo, shape):
        """(tsdf bits, weight bits) of the samples lo .. lo + shape - 1, two (nz,ny,nx) uint32 arrays."""
        nx, ny, nz = shape
        t = np.full((nz, ny, nx), ONE_BITS, np.uint32)
        w = np.zeros((nz, ny, nx), np.uint32)
        for (i, j, k), (tb, wb) in self.samples.items():
            if lo[0] <= i < lo[0] + nx and lo[1] <= j < lo[1] + ny and lo[2] <= k < lo[2] + nz:
                t[k - lo[2], j - lo[1], i - lo[0]], w[k - lo[2], j - lo[1], i - lo[0]] = tb, wb
        return t, w

    def check(self, base, shape, tsdf, weight, store):
        """window (ring storage) and store (brick -> (tsdf, weight)) together are this world: every window sample, every stored brick,
        and nothing written is missing from both."""
        wt, ww = self.block(base, shape)
        assert np.array_equal(bits(WR.to_block(tsdf, base)), wt) and np.array_equal(bits(WR.to_block(weight, base)), ww), "window"
        inside = set(window_bricks(base, shape))
        assert not inside & set(store), "a brick in the window and in the store"
        for key, (t, w) in store.items():
            bt, bw = self.block(tuple(8 * k for k in key), (8, 8, 8))
            assert np.array_equal(bits(t), bt) and np.array_equal(bits(w), bw), key
            assert brick_differs(t, w), "an empty brick is stored: %s" % (key,)
        for (i, j, k), (tb, wb) in self.samples.items():
            if (tb, wb) != (int(ONE_BITS), 0):
                key = (i // 8, j // 8, k // 8)
                assert key in inside or key in store, "sample %s is lost" % ((i, j, k),)


# ---- the library on CPU tensors ------------------------------------------------------------------------------------------------------
def _arr(ptr, count, ctype=C.c_float):
    addr = getattr(ptr, "value", ptr)
    return np.ctypeslib.as_array((ctype * int(count)).from_address(addr))


class HostLib(object):
    """The four calls of a rolling window with a store, by their statements, on host memory.  `calls` lists the names in order."""

    def __init__(self):
        self.calls = []

    def _window(self, t, w, nx, ny, nz):
        return _arr(t, nx * ny * nz).reshape(nz, ny, nx), _arr(w, nx * ny * nz).reshape(nz, ny, nx)

    def ovn_tsdf_window_shift(self, ctx, stream, t, w, nx, ny, nz, old_base, new_base):
        self.calls.append("ovn_tsdf_window_shift")
        tt, ww = self._window(t, w, nx, ny, nz)
        tt[...], ww[...], _ = WR.shift(tt.copy(), ww.copy(), tuple(old_base), tuple(new_base))
        return 0

    def ovn_tsdf_window_brick_flags(self, ctx, stream, t, w, nx, ny, nz, base, lo, hi, flags):
        self.calls.append("ovn_tsdf_window_brick_flags")
        tt, ww = self._window(t, w, nx, ny, nz)
        base, lo, hi = tuple(base), tuple(lo), tuple(hi)
        assert all(b <= 8 * l <= 8 * h <= b + n for b, l, h, n in zip(base, lo, hi, (nx, ny, nz))), "box outside the window"
        keys = [(x, y, z) for z in range(lo[2], hi[2]) for y in range(lo[1], hi[1]) for x in range(lo[0], hi[0])]
        if keys:
            out = _arr(flags, len(keys), C.c_uint8)
            for i, key in enumerate(keys):
                ix = _brick_index(key, tt.shape)
                out[i] = brick_differs(tt[ix], ww[ix])
        return 0

    def _page(self, name, out, t, w, nx, ny, nz, base, n, bricks, slots, pool):
        self.calls.append(name)
        tt, ww = self._window(t, w, nx, ny, nz)
        if n == 0:
            return 0
        keys, sl = _arr(bricks, 3 * n, C.c_int32).reshape(n, 3), _arr(slots, n, C.c_int32)
        words = _arr(pool, (int(sl.max()) + 1) * 1024)
        inside = set(window_bricks(tuple(base), (nx, ny, nz)))
        for key, s in zip(keys.tolist(), sl.tolist()):
            assert tuple(key) in inside and s >= 0, "brick %s outside the window" % (key,)
            ix = _brick_index(key, tt.shape)
            home = words[s * 1024:(s + 1) * 1024]
            if out:
                home[:512], home[512:] = tt[ix].ravel(), ww[ix].ravel()
            else:
                tt[ix], ww[ix] = home[:512].reshape(8, 8, 8), home[512:].reshape(8, 8, 8)
        return 0

    def ovn_tsdf_window_page_out(self, ctx, stream, *a):
        return self._page("ovn_tsdf_window_page_out", True, *a)

    def ovn_tsdf_window_page_in(self, ctx, stream, *a):
        return self._page("ovn_tsdf_window_page_in", False, *a)


def moves_to(start, steps):
    """The bases a window visits from `start` under the relative `steps`."""
    out, b = [], tuple(start)
    for s in steps:
        b = tuple(x + d for x, d in zip(b, s))
        out.append(b)
    return out


def position_for(volume, new_base):
    """A position whose `follow` brings `volume` to new_base (a move by multiples of its shift): the middle of the centre cell."""
    n = volume.shape
    return np.asarray(volume.anchor) + (np.asarray(new_base) + np.asarray([v // 2 for v in n]) + 0.5) * volume.voxel
