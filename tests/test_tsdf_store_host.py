"""CPU: the brick store behind the rolling TSDF window (overlapnet_amd/tsdf_store.py, include/ovn_hip_tsdf_store.h; DESIGN.md section
38) as far as it goes without a GPU: the ledger of the new header and of `_lib.STORE_SIGNATURES`, the wrappers' arguments and refusals,
the library's own argument errors, the NumPy model of tests/_tsdf_store_ref.py against a world that never forgets -- and, on the
stand-in library of that file, `TsdfBrickStore` and `RollingTsdfVolume(store=True)` themselves against the same world -- slot reuse,
the cap, save and load, and the tiles of the mesh sweep."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _tsdf_store_ref as SR
import _tsdf_window_ref as WR
from overlapnet_amd import _lib
from overlapnet_amd import engine as E
from overlapnet_amd import tsdf
from overlapnet_amd import tsdf_store as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ovn_hip_tsdf_store.h")
HANDLE, STREAM = 0x1000, 0x2000
NAMES = ["ovn_tsdf_window_brick_flags", "ovn_tsdf_window_page_in", "ovn_tsdf_window_page_out"]
SHAPE = (16, 24, 16)                            # the lattice of the model's runs
BASES = [(40, 8, 8), (-32, -16, -8)]


# ---- the ledger of include/ovn_hip_tsdf_store.h ---------------------------------------------------------------------------------------
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double,
            "uint8_t": C.c_uint8}


def _header_text():
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


def _header_prototypes():
    """name -> (return type, [(parameter type, parameter name)]) as the header spells them."""
    out = {}
    for ret, name, params in re.findall(r"\b(int|int64_t|const char\*)\s+(ovn_\w+)\s*\(([^;{}]*?)\)\s*;", _header_text(), flags=re.S):
        types = []
        for p in (" ".join(p.split()) for p in params.split(",")):
            if p == "void":
                continue
            m = re.match(r"^(.*?[\s*])(\w+)$", p)
            assert m, "%s: parameter %r has no name" % (name, p)
            types.append((m.group(1).strip(), m.group(2)))
        out[name] = (ret, types)
    return out


def _ctypes_accepted(ctype):
    base = " ".join(ctype.replace("const", " ").replace("*", " ").split())
    depth = ctype.count("*")
    if depth == 0:
        return [_SCALARS[base]]
    assert depth == 1, ctype
    if base in ("ovn_ctx", "void"):
        return [C.c_void_p]
    return [C.POINTER(_SCALARS[base]), C.c_void_p]


def test_library_exports_the_store_header():
    _lib.build()
    lib = C.CDLL(_lib.LIB_PATH)
    names = sorted(set(re.findall(r"\b(ovn_[a-z0-9_]+)\s*\(", _header_text())))
    assert names == NAMES
    for n in names:
        assert hasattr(lib, n), "libovn_hip.so does not export %s declared in include/ovn_hip_tsdf_store.h" % n
    assert sorted(_lib.STORE_SIGNATURES) == names
    assert '#include "ovn_hip.h"' in open(HEADER).read()
    bound = _lib.load()                                       # load() binds the third table in the same loop
    for n in names:
        assert getattr(bound, n).argtypes == _lib.STORE_SIGNATURES[n][1] and getattr(bound, n).restype is C.c_int


def test_store_signatures_have_the_types_of_the_header():
    protos = _header_prototypes()
    assert sorted(protos) == sorted(_lib.STORE_SIGNATURES)
    tables = [set(_lib.SIGNATURES), set(_lib.EXT_SIGNATURES), set(_lib.STORE_SIGNATURES)]
    assert not tables[0] & tables[1] and not tables[0] & tables[2] and not tables[1] & tables[2]
    assert sorted(_lib.EXT_SIGNATURES) == ["ovn_deskew"]
    wrong = []
    for name, (ret, params) in protos.items():
        res, args = _lib.STORE_SIGNATURES[name]
        if res is not _SCALARS[ret]:
            wrong.append("%s returns %s, STORE_SIGNATURES says %s" % (name, ret, res.__name__))
        if len(args) != len(params):
            wrong.append("%s takes %d parameters, STORE_SIGNATURES lists %d" % (name, len(params), len(args)))
            continue
        for i, ((c, _), a) in enumerate(zip(params, args)):
            if not any(a is ok for ok in _ctypes_accepted(c)):
                wrong.append("%s parameter %d is %s, STORE_SIGNATURES says %s" % (name, i, c, a.__name__))
        assert [n for _, n in params][:2] == ["ctx", "stream"], name
    assert not wrong, "\n".join(wrong)


def test_a_missing_store_symbol_is_the_usual_error(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.STORE_SIGNATURES, "ovn_no_such_call", (C.c_int, []))
    with pytest.raises(_lib.OvnError, match="does not export ovn_no_such_call"):
        _lib.load()


def test_argument_errors_of_the_library_without_a_gpu():
    """Every refusal comes before the context is read or anything is launched: a context that is no context and buffers that are no
    device memory get as far as the checks and no further."""
    lib = _lib.load()
    i3 = lambda v: (C.c_int32 * 3)(*v)
    room = (C.c_char * 64)()
    ctx = C.c_void_p(C.addressof(room))
    buf = C.c_void_p(0x10000)                                  # aligned, never followed
    nx, ny, nz = WR.SHAPE
    base = i3(WR.BASE)
    lo, hi = i3((5, 1, 1)), i3((6, 2, 2))
    flags = lambda c, t, w, b, l, h, f=buf, dims=(nx, ny, nz): lib.ovn_tsdf_window_brick_flags(c, None, t, w, dims[0], dims[1], dims[2], b, l, h, f)
    err = lambda: lib.ovn_last_error()
    assert flags(None, buf, buf, base, lo, hi) == 1 and b"ctx is NULL" in err()
    assert flags(ctx, None, buf, base, lo, hi) == 1 and b"NULL" in err()
    assert flags(ctx, buf, buf, i3((44, 8, 8)), lo, hi) == 1 and b"multiples of 8" in err()              # an unaligned base
    assert flags(ctx, buf, buf, base, lo, hi, dims=(70, ny, nz)) == 1 and b"multiples of 8" in err()
    assert flags(ctx, C.c_void_p(0x10004), buf, base, lo, hi) == 1 and b"16-byte" in err()
    for blo, bhi in (((4, 1, 1), (6, 2, 2)), ((5, 1, 1), (15, 2, 2)), ((5, 1, 1), (6, 5, 2)), ((5, 0, 1), (6, 2, 2)), ((6, 1, 1), (5, 2, 2)),
                     ((5, 1, 1), (6, 2, 4))):                                                             # a box outside the window
        assert flags(ctx, buf, buf, base, i3(blo), i3(bhi)) == 1 and b"outside the window" in err(), (blo, bhi)
    assert flags(ctx, buf, buf, base, lo, hi, f=None) == 1 and b"flags is NULL" in err()
    assert flags(ctx, buf, buf, base, lo, lo, f=None) == 0                                                # an empty box: no launch
    for name in ("ovn_tsdf_window_page_out", "ovn_tsdf_window_page_in"):
        fn = getattr(lib, name)
        page = lambda c, t, b, n, lists=buf, pool=buf: fn(c, None, t, buf, nx, ny, nz, b, n, lists, lists, pool)
        assert page(None, buf, base, 1) == 1 and b"ctx is NULL" in err()
        assert page(ctx, buf, base, -1) == 1 and b"< 0" in err()
        assert page(ctx, buf, i3((40, 8, 12)), 1) == 1 and b"multiples of 8" in err()
        assert page(ctx, buf, i3(((1 << 20) - 64, 8, 8)), 1) == 1 and b"2^20" in err()
        assert page(ctx, None, base, 1) == 1
        assert page(ctx, buf, base, 1, lists=None) == 1 and b"NULL bricks" in err()
        assert page(ctx, buf, base, 1, pool=C.c_void_p(0x10008)) == 1 and b"16-byte" in err()
        assert page(ctx, buf, base, 0, lists=None, pool=None) == 0                                         # n == 0: no launch


# ---- the wrappers ----------------------------------------------------------------------------------------------------------------------
def _fake_engine(lib):
    e = E.OvnEngine.__new__(E.OvnEngine)
    e.lib = lib
    e.device_index = 0
    e.device = torch.device("cpu")
    e._h = C.c_void_p(HANDLE)
    e._dev = lambda: contextlib.nullcontext()
    e._stream = lambda: C.c_void_p(STREAM)
    return e


class Recorder:
    """Stands in for the CDLL: a store call checks its arguments against STORE_SIGNATURES as ctypes would, notes the call, returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name not in _lib.STORE_SIGNATURES:
            raise AttributeError(name)
        res, argtypes = _lib.STORE_SIGNATURES[name]

        def fn(*args):
            assert len(args) == len(argtypes), "%s takes %d arguments, the wrapper passes %d" % (name, len(argtypes), len(args))
            for i, (t, a) in enumerate(zip(argtypes, args)):
                try:
                    t.from_param(a)
                except (TypeError, C.ArgumentError) as exc:
                    raise AssertionError("%s: argument %d (%r) is no %s: %s" % (name, i, a, t.__name__, exc))
            self.calls.append((name, args))
            return 0
        return fn


def _inputs(n=3):
    nx, ny, nz = WR.SHAPE
    return dict(tsdf=torch.ones(nz, ny, nx), weight=torch.zeros(nz, ny, nx), bricks=torch.zeros(n, 3, dtype=torch.int32),
                slots=torch.arange(n, dtype=torch.int32), pool=torch.zeros(4 * 1024), flags=torch.zeros(2 * 3 * 9, dtype=torch.uint8))


def _value(v):
    if isinstance(v, C.Array):
        return list(v)
    return getattr(v, "value", v)


def test_wrappers_pass_the_header_arguments_in_order():
    rec = Recorder()
    eng = _fake_engine(rec)
    a = _inputs()
    protos = _header_prototypes()
    nx, ny, nz = WR.SHAPE
    out = S.window_brick_flags(eng, a["tsdf"], a["weight"], WR.BASE, (5, 1, 1), (14, 4, 3))
    same = S.window_brick_flags(eng, a["tsdf"], a["weight"], WR.BASE, (5, 1, 1), (14, 4, 3), out=a["flags"])
    assert tuple(out.shape) == (2, 3, 9) and out.dtype == torch.uint8 and same is a["flags"]
    names = [n for _, n in protos["ovn_tsdf_window_brick_flags"][1]]
    assert names == ["ctx", "stream", "tsdf_dev", "weight_dev", "nx", "ny", "nz", "base", "box_lo", "box_hi", "flags_dev"]
    got = dict(zip(names, (_value(v) for v in rec.calls[1][1])))
    assert got == dict(ctx=HANDLE, stream=STREAM, tsdf_dev=a["tsdf"].data_ptr(), weight_dev=a["weight"].data_ptr(), nx=nx, ny=ny, nz=nz,
                       base=list(WR.BASE), box_lo=[5, 1, 1], box_hi=[14, 4, 3], flags_dev=a["flags"].data_ptr())
    for call, wrapper in (("ovn_tsdf_window_page_out", S.window_page_out), ("ovn_tsdf_window_page_in", S.window_page_in)):
        wrapper(eng, a["tsdf"], a["weight"], WR.BASE_NEG, a["bricks"], a["slots"], a["pool"])
        names = [n for _, n in protos[call][1]]
        assert names == ["ctx", "stream", "tsdf_dev", "weight_dev", "nx", "ny", "nz", "base", "n", "bricks_dev", "slots_dev", "pool_dev"]
        name, args = rec.calls[-1]
        assert name == call and dict(zip(names, (_value(v) for v in args))) == dict(
            ctx=HANDLE, stream=STREAM, tsdf_dev=a["tsdf"].data_ptr(), weight_dev=a["weight"].data_ptr(), nx=nx, ny=ny, nz=nz,
            base=list(WR.BASE_NEG), n=3, bricks_dev=a["bricks"].data_ptr(), slots_dev=a["slots"].data_ptr(), pool_dev=a["pool"].data_ptr())
    assert len(rec.calls) == 4


TENSORS = [("flags", a) for a in ("tsdf", "weight", "flags")] + [(c, a) for c in ("page_out", "page_in")
                                                                 for a in ("tsdf", "weight", "bricks", "slots", "pool")]


@pytest.mark.parametrize("call, arg", TENSORS, ids=["%s-%s" % t for t in TENSORS])
@pytest.mark.parametrize("kind", ["dtype", "device", "contiguity", "shape"])
def test_wrappers_refuse_bad_tensors_before_the_library(call, arg, kind):
    rec = Recorder()
    eng = _fake_engine(rec)
    a = _inputs()
    t = a[arg]
    if kind == "dtype":
        bad = t.to(torch.float64)
    elif kind == "device":
        bad = t.to("meta")
    elif kind == "contiguity":
        wide = torch.zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],), dtype=t.dtype)
        bad = wide[..., ::2]
        assert not bad.is_contiguous() and bad.shape == t.shape
    else:
        bad = torch.zeros((t.shape[0] + 1,) + tuple(t.shape[1:]), dtype=t.dtype)
        if arg == "tsdf":                        # a tsdf of another shape: the weight no longer matches it
            bad = torch.ones(t.shape[0], t.shape[1], t.shape[2] + 8)
    a[arg] = bad
    with pytest.raises(_lib.OvnError):
        if call == "flags":
            S.window_brick_flags(eng, a["tsdf"], a["weight"], WR.BASE, (5, 1, 1), (14, 4, 3), out=a["flags"])
        else:
            getattr(S, "window_" + call)(eng, a["tsdf"], a["weight"], WR.BASE, a["bricks"], a["slots"], a["pool"])
    assert rec.calls == []


# ---- the model against a world that never forgets ------------------------------------------------------------------------------------
SEQUENCES = {
    "x8": [(8, 0, 0), (-8, 0, 0), (-8, 0, 0), (8, 0, 0)],
    "x16": [(16, 0, 0), (-16, 0, 0), (0, -16, 0), (0, 16, 0), (0, 0, 16), (0, 0, -16)],
    "mixed": [(8, -8, 0), (-16, 8, 8), (0, 16, -8), (8, -16, 0), (8, 8, 8), (-8, -8, -8)],
    "whole": [(16, 0, 0), (-16, 0, 0), (0, 24, 0), (0, -24, 0), (0, 0, -16), (0, 0, 16)],
    "more": [(48, 0, 0), (-80, 32, 0), (32, -32, 0), (8, 40, -24), (-8, -40, 24)],
    "there_and_back": [(8, 0, 0), (16, 8, 0), (32, 0, 8), (-32, 0, -8), (-16, -8, 0), (-8, 0, 0)],
}


def _writes(g, base, count=40):
    """Random samples inside the window at `base`: (index, tsdf, weight), among them the two that only their bits give away."""
    out = []
    for _ in range(count):
        idx = tuple(int(b + g.integers(0, n)) for b, n in zip(base, SHAPE))
        out.append((idx, float(g.uniform(-1, 1)), float(g.integers(1, 9))))
    out.append((tuple(b + 1 for b in base), 0.5, 0.0))                          # weight 0, tsdf != 1
    out.append((tuple(b + n - 2 for b, n in zip(base, SHAPE)), 1.0, -0.0))      # tsdf 1, weight -0.0
    return out


@pytest.mark.parametrize("base", BASES, ids=["positive", "negative"])
@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_model_window_and_store_are_the_world(name, base):
    g = np.random.default_rng(2 * sorted(SEQUENCES).index(name) + BASES.index(base))
    model, world = SR.Model(SHAPE, base), SR.World()
    for new in [base] + SR.moves_to(base, SEQUENCES[name]):
        model.move(new)
        world.check(model.base, SHAPE, model.tsdf, model.weight, model.store)
        for idx, t, w in _writes(g, new):
            model.write(idx, t, w)
            world.write(idx, t, w)
        world.check(model.base, SHAPE, model.tsdf, model.weight, model.store)
    assert len(world.samples) > 100


def _volume(lib, base, **kw):
    """A RollingTsdfVolume of SHAPE at `base` on CPU tensors and the stand-in library."""
    eng = _fake_engine(lib)
    vol = tsdf.RollingTsdfVolume(eng, tuple(float(n) for n in SHAPE), 1.0, **kw)
    assert vol.shape == SHAPE
    vol.base = tuple(base)
    return vol


def _store_dict(store):
    return {k: store.get(k) for k in store.bricks()}


@pytest.mark.parametrize("base", BASES, ids=["positive", "negative"])
@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_volume_with_a_store_is_the_model_and_the_world(name, base):
    """`RollingTsdfVolume(store=True).follow` on the stand-in library: after every move and every write, window and store have the
    model's bits and are the world."""
    g = np.random.default_rng(2 * sorted(SEQUENCES).index(name) + BASES.index(base))
    lib = SR.HostLib()
    vol = _volume(lib, base, store=True)
    model, world = SR.Model(SHAPE, base), SR.World()
    for new in SR.moves_to(base, SEQUENCES[name]):
        for idx, t, w in _writes(g, vol.base):
            model.write(idx, t, w)
            world.write(idx, t, w)
            s = tuple(int(WR.slots_of(i, n)) for i, n in zip(idx, SHAPE))
            vol.tsdf[s[2], s[1], s[0]], vol.weight[s[2], s[1], s[0]] = t, w
        del lib.calls[:]
        assert vol.follow(SR.position_for(vol, new)) and vol.base == new
        assert lib.calls[0] == "ovn_tsdf_window_brick_flags" and "ovn_tsdf_window_shift" in lib.calls
        model.move(new)
        held = _store_dict(vol.store)
        assert sorted(held) == sorted(model.store) and len(vol.store) == len(held) and vol.store.bytes == 4096 * len(held)
        for k in held:
            assert np.array_equal(SR.bits(held[k][0]), SR.bits(model.store[k][0])) and np.array_equal(SR.bits(held[k][1]), SR.bits(model.store[k][1]))
        assert np.array_equal(SR.bits(vol.tsdf.numpy()), SR.bits(model.tsdf)) and np.array_equal(SR.bits(vol.weight.numpy()), SR.bits(model.weight))
        world.check(vol.base, SHAPE, vol.tsdf.numpy(), vol.weight.numpy(), held)
    assert vol.pieces == [] and vol.n_shifts == len(SEQUENCES[name])
    vol.reset()
    assert len(vol.store) == 0 and vol.store.bricks() == []


def test_without_a_store_the_calls_are_those_of_before():
    lib = SR.HostLib()
    vol = _volume(lib, BASES[0])
    assert vol.store is None
    vol.tsdf[3, 3, 3] = 0.25
    assert vol.follow(SR.position_for(vol, (48, 8, 8)))
    assert lib.calls == ["ovn_tsdf_window_shift"]                      # n_scans == 0: nothing is meshed either
    with pytest.raises(ValueError, match="on_leave"):
        _volume(lib, BASES[0], store=True).follow((0, 0, 0), on_leave=lambda p: None)
    with pytest.raises(ValueError, match="store must be"):
        _volume(lib, BASES[0], store="yes")


# ---- slots and the cap -----------------------------------------------------------------------------------------------------------------
def _plant(vol, keys, value=0.5):
    """One sample of each listed brick of the window set to `value`."""
    for key in keys:
        s = tuple(int(WR.slots_of(8 * k + 3, n)) for k, n in zip(key, SHAPE))
        vol.tsdf[s[2], s[1], s[0]] = value


def test_free_slots_are_reused_in_ascending_order():
    lib = SR.HostLib()
    base = (0, 0, 0)
    vol = _volume(lib, base, store=True)
    store = vol.store
    col = [(0, j, k) for k in range(2) for j in range(3)]               # the six bricks of the x = 0 .. 7 slab, ascending (z, y, x)
    _plant(vol, col)
    vol.follow(SR.position_for(vol, (8, 0, 0)))
    assert [store._index[k] for k in col] == [0, 1, 2, 3, 4, 5] and store._top == 6 and store._free == []
    vol.follow(SR.position_for(vol, (0, 0, 0)))                         # back: all six return, their slots are free
    assert len(store) == 0 and sorted(store._free) == [0, 1, 2, 3, 4, 5]
    three = [col[1], col[3], col[4]]
    for key in col:
        if key not in three:                                            # empty three of them by hand
            ix = SR._brick_index(key, vol.tsdf.shape)
            vol.tsdf.numpy()[ix] = 1.0
    vol.follow(SR.position_for(vol, (8, 0, 0)))
    assert [store._index[k] for k in three] == [0, 1, 2] and sorted(store._free) == [3, 4, 5] and store._top == 6
    # more bricks than free slots: the free ones first, ascending, then new ones
    vol.follow(SR.position_for(vol, (0, 8, 0)))                         # (0,1,0) and (0,1,1) come back: slots 0 and 2 are free again
    assert sorted(store._free) == [0, 2, 3, 4, 5] and sorted(store._index.values()) == [1]
    _plant(vol, SR.window_bricks(vol.base, SHAPE), 0.75)
    vol.follow(SR.position_for(vol, (64, 64, 64)))                      # the whole window leaves: 12 bricks
    assert len(store) == 13 and sorted(store._index.values()) == list(range(13)) and store._free == []
    order = sorted(SR.window_bricks((0, 8, 0), SHAPE), key=lambda k: (k[2], k[1], k[0]))
    assert [store._index[k] for k in order] == [0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12]
    assert store.capacity >= 13


def test_a_page_out_over_the_cap_raises_and_changes_nothing():
    lib = SR.HostLib()
    vol = _volume(lib, (0, 0, 0))
    store = S.TsdfBrickStore(vol.engine, max_bytes=4 * 4096)
    vol = _volume(lib, (0, 0, 0), store=store)
    _plant(vol, [(0, 0, 0), (0, 1, 0), (0, 2, 1)])
    vol.follow(SR.position_for(vol, (8, 0, 0)))
    assert len(store) == 3
    _plant(vol, [(1, 0, 0), (1, 1, 1)])                                  # two more would make five
    before = (vol.tsdf.clone(), vol.weight.clone(), vol.base, dict(store._index), list(store._free), store._top, store._pool.clone())
    with pytest.raises(_lib.OvnError, match="max_bytes"):
        vol.follow(SR.position_for(vol, (16, 0, 0)))
    assert torch.equal(vol.tsdf, before[0]) and torch.equal(vol.weight, before[1]) and vol.base == before[2] == (8, 0, 0)
    assert store._index == before[3] and store._free == before[4] and store._top == before[5] and torch.equal(store._pool, before[6])
    assert "ovn_tsdf_window_shift" not in lib.calls[lib.calls.index("ovn_tsdf_window_shift") + 1:]     # the one shift is the first move's
    vol.follow(SR.position_for(vol, (8, 8, 0)))                          # a move that keeps one brick still fits
    assert len(store) == 4
    with pytest.raises(ValueError, match="max_bytes"):
        S.TsdfBrickStore(vol.engine, max_bytes=100)


# ---- a file ------------------------------------------------------------------------------------------------------------------------------
def _filled(lib, anchor=(1.0, -2.0, 0.5)):
    vol = _volume(lib, (0, 0, 0), store=True, anchor=anchor)
    g = np.random.default_rng(5)
    vol.tsdf.copy_(torch.from_numpy(g.uniform(-1, 1, vol.tsdf.shape).astype(np.float32)))
    vol.weight.copy_(torch.from_numpy(g.integers(0, 5, vol.weight.shape).astype(np.float32)))
    vol.follow(SR.position_for(vol, (64, 64, 64)))
    return vol


def test_save_and_load_round_trip_in_bytes(tmp_path):
    lib = SR.HostLib()
    vol = _filled(lib)
    a, b, c = (str(tmp_path / n) for n in ("a.npz", "b.npz", "c.npz"))
    vol.store.save(a)
    loaded = S.TsdfBrickStore.load(vol.engine, a)
    assert loaded.bricks() == vol.store.bricks() and len(loaded) == 12 and loaded.meta["voxel"] == 1.0
    assert np.array_equal(loaded.meta["anchor"], [1.0, -2.0, 0.5]) and loaded.meta["trunc"] == 4.0 and loaded.meta["max_weight"] == 64.0
    for k in loaded.bricks():
        for x, y in zip(loaded.get(k), vol.store.get(k)):
            assert np.array_equal(SR.bits(x), SR.bits(y))
    loaded.save(b)
    assert open(a, "rb").read() == open(b, "rb").read()
    # equal content in other slots, written at another time, is the same file
    again = _filled(SR.HostLib())
    s = again.store
    keys = s.bricks()
    moved = dict(zip(keys, [s._index[k] for k in reversed(keys)]))
    pool = s._pool.clone()
    for k in keys:
        pool[moved[k] * 1024:(moved[k] + 1) * 1024] = s._pool[s._index[k] * 1024:(s._index[k] + 1) * 1024]
    s._pool, s._index = pool, moved
    s.save(c)
    assert open(a, "rb").read() == open(c, "rb").read()
    with np.load(a) as z:
        assert sorted(z.files) == ["anchor", "keys", "max_weight", "payload", "trunc", "voxel"]
        assert z["keys"].dtype == np.int32 and z["payload"].shape == (12, 1024) and z["keys"].tolist() == sorted(z["keys"].tolist())


def test_a_loaded_store_continues_only_on_its_lattice(tmp_path):
    lib = SR.HostLib()
    vol = _filled(lib)
    path = str(tmp_path / "map.npz")
    vol.store.save(path)
    before = {k: vol.store.get(k) for k in vol.store.bricks()}
    for bad in (dict(anchor=(1.0, -2.0, 0.75)), dict(anchor=(1.0, -2.0, 0.5), trunc=3.0)):
        with pytest.raises(ValueError, match="lattice"):
            _volume(lib, (0, 0, 0), store=S.TsdfBrickStore.load(vol.engine, path), **bad)
    with pytest.raises(ValueError, match="voxel"):
        tsdf.RollingTsdfVolume(vol.engine, (8.0, 12.0, 8.0), 0.5, anchor=(1.0, -2.0, 0.5), store=S.TsdfBrickStore.load(vol.engine, path))
    cont = _volume(lib, (64, 64, 64), store=S.TsdfBrickStore.load(vol.engine, path), anchor=(1.0, -2.0, 0.5))
    cont.follow(SR.position_for(cont, (0, 0, 0)))                       # the window returns to the saved region: it holds the saved bits
    assert len(cont.store) == 0
    for k, (t, w) in before.items():
        ix = SR._brick_index(k, cont.tsdf.shape)
        assert np.array_equal(SR.bits(cont.tsdf.numpy()[ix]), SR.bits(t)) and np.array_equal(SR.bits(cont.weight.numpy()[ix]), SR.bits(w))
    with pytest.raises(_lib.OvnError, match="no volume"):
        S.TsdfBrickStore(vol.engine).save(path)


# ---- the tiles of the mesh sweep -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(16, 16, 16), (24, 16, 32)])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_sweep_tiles_own_every_cell_exactly_once(shape, seed):
    g = np.random.default_rng(seed)
    keys = sorted(set((int(x), int(y), int(z)) for x, y, z in g.integers(-6, 7, (25, 3))))
    if seed == 2:
        keys = [keys[0]]                                                # a single brick
    tiles = S.sweep_tiles(keys, shape)
    lo = np.min(np.asarray(keys), axis=0) * 8
    hi = (np.max(np.asarray(keys), axis=0) + 1) * 8
    samples = np.zeros(tuple(hi - lo)[::-1], bool)                      # which samples of the bounding box lie in a brick
    for k in keys:
        o = np.asarray(k) * 8 - lo
        samples[o[2]:o[2] + 8, o[1]:o[1] + 8, o[0]:o[0] + 8] = True
    owners = np.zeros(tuple(hi - lo + 8)[::-1], np.int64)               # per cell low corner lo - 8 .. hi - 1, offset by 8
    assert [t[0] for t in tiles] == sorted((t[0] for t in tiles), key=lambda b: (b[2], b[1], b[0]))
    for base, clo, chi, tkeys in tiles:
        assert all(b % 8 == 0 for b in base) and clo == base
        assert all(b <= l and h + 1 <= b + n for b, l, h, n in zip(base, clo, chi, shape))          # the far corners are the tile's
        assert all(h - l == n - 8 for l, h, n in zip(clo, chi, shape))
        want = [k for k in keys if all(b < 8 * v + 8 and 8 * v < b + n for v, b, n in zip(k, base, shape))]
        assert tkeys == sorted(want, key=lambda k: (k[2], k[1], k[0])) and tkeys
        a, b = np.asarray(clo) - lo + 8, np.asarray(chi) - lo + 8
        a, b = np.maximum(a, 0), np.minimum(b, hi - lo + 8)
        owners[a[2]:b[2], a[1]:b[1], a[0]:b[0]] += 1
    assert owners.max() == 1
    # brute force: a cell with a corner in some brick and its low corner at or past lo is owned by exactly one tile
    near = np.zeros_like(owners, bool)
    pad = np.zeros(tuple(hi - lo + 9)[::-1], bool)
    pad[8:-1, 8:-1, 8:-1] = samples
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                near |= pad[dz:dz + near.shape[0], dy:dy + near.shape[1], dx:dx + near.shape[2]]
    inside = np.zeros_like(near)
    inside[8:, 8:, 8:] = True
    assert near[inside].any() and np.all(owners[near & inside] == 1)
    assert S.sweep_tiles([], shape) == []
