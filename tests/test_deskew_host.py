"""CPU: the motion compensation of raw sweeps (overlapnet_amd/deskew.py, include/ovn_hip_deskew.h) as far as
it goes without a GPU: the SE(3) helpers, the bent-scan generator and the sign conventions of tests/_deskew_ref.py, the float32
restatement against the error bound the GPU test uses, every Python-level refusal, and the ledger of the extension header -- the library
exports what include/ovn_hip_deskew.h declares, `_lib.EXT_SIGNATURES` mirrors it one to one, and `deskew_scans` hands the library the
header's arguments in the header's order and refuses a bad tensor before the library is reached."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _deskew_ref as DR
from overlapnet_amd import _lib
from overlapnet_amd import deskew as D
from overlapnet_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ovn_hip_deskew.h")
HANDLE, STREAM = 0x1000, 0x2000


# ---- SE(3) ----------------------------------------------------------------------------------------------------------------------------
ANGLES = [0.0, 1e-12, 1e-9, 1e-5, 0.05, 0.0999, D.SERIES_BELOW, 0.1001, 0.5, 1.0, 2.0, 3.0, np.pi - 0.1]


@pytest.mark.parametrize("mod", [D, DR], ids=["package", "reference"])
def test_exp_and_log_are_inverse_to_1e_12(mod):
    g = np.random.default_rng(3)
    for th in ANGLES:
        for _ in range(8):
            k = g.normal(size=3)
            xi = np.concatenate([g.normal(size=3) * 3.0, k / np.linalg.norm(k) * th])
            t = mod.se3_exp(xi)
            assert np.abs(t[:3, :3] @ t[:3, :3].T - np.eye(3)).max() < 1e-12 and np.array_equal(t[3], [0, 0, 0, 1])
            assert np.abs(mod.se3_log(t) - xi).max() < 1e-12, th
            assert np.abs(mod.se3_exp(mod.se3_log(t)) - t).max() < 1e-12, th
    assert np.array_equal(mod.se3_exp(np.zeros(6)), np.eye(4)) and np.array_equal(mod.se3_log(np.eye(4)), np.zeros(6))


def test_package_and_reference_agree_and_compose():
    g = np.random.default_rng(4)
    for th in ANGLES:
        xi = np.concatenate([g.normal(size=3), g.normal(size=3)])
        xi[3:] *= th / np.linalg.norm(xi[3:])
        assert np.abs(D.se3_exp(xi) - DR.se3_exp(xi)).max() < 1e-12
        assert np.abs(D.se3_exp(0.3 * xi) @ D.se3_exp(0.7 * xi) - D.se3_exp(xi)).max() < 1e-12       # one-parameter subgroup


def test_twists_from_poses_on_a_screw_motion():
    xi = np.array([0.5, 0.02, -0.01, 0.003, -0.002, 0.026])
    start = DR.se3_exp([1.0, -2.0, 0.5, 0.2, 0.1, -0.4])
    poses = np.stack([start @ D.se3_exp(k * xi) for k in range(6)])
    tw = D.twists_from_poses(poses)
    assert tw.shape == (6, 6) and np.abs(tw - xi[None]).max() < 1e-12
    assert np.array_equal(D.twists_from_poses(poses[:1]), np.zeros((1, 6))) and D.twists_from_poses(poses[:0]).shape == (0, 6)
    with pytest.raises(ValueError):
        D.twists_from_poses(np.eye(4))


# ---- the generator, the reference and the signs ---------------------------------------------------------------------------------------
def test_reference_deskew_brings_a_bent_scan_back_to_its_hits():
    pose, xi, pts, times, hits = DR.kernel_scan()
    assert pts.shape[0] > 0.5 * 16 * 180 and len(np.unique(times)) == 6 and times.dtype == np.float32
    one = np.concatenate([pts[:, :3].astype(np.float64), np.ones((pts.shape[0], 1))], 1)
    fixed = DR.deskew(pts, times, xi, 0.5)
    back = np.concatenate([fixed[:, :3], np.ones((pts.shape[0], 1))], 1)
    err = np.linalg.norm((pose @ back.T).T[:, :3] - hits, axis=1)
    off = np.linalg.norm((pose @ one.T).T[:, :3] - hits, axis=1)
    # what the twist predicts for a point left as it is: |Exp(tau xi) p - p|
    want = np.array([np.linalg.norm((D.se3_exp((float(s) - 0.5) * xi) @ q)[:3] - q[:3]) for s, q in zip(times, one)])
    print("bent 16 x 180 scan: %d points, deskewed within %.2e m of their hits, raw off by up to %.3f m" % (pts.shape[0], err.max(), off.max()))
    assert err.max() < 1e-9
    assert np.abs(off - want).max() < 1e-9
    assert off.max() > 0.8 * (5.0 / 12.0) * np.linalg.norm(xi[:3])           # the outer slices sit 5/12 of a sweep from t_ref
    assert np.array_equal(fixed[:, 3], pts[:, 3].astype(np.float64))
    # the wrong sign of tau or the inverse transform doubles the error instead of removing it
    wrong = DR.deskew(pts, times, -xi, 0.5)
    wrong = np.concatenate([wrong[:, :3], np.ones((pts.shape[0], 1))], 1)
    assert np.linalg.norm((pose @ wrong.T).T[:, :3] - hits, axis=1).max() > 1.5 * off.max()


def test_reference_special_cases():
    pts = np.array([[1.0, 2.0, 3.0, 0.5], [-0.0, 4.0, -1.0, 0.25], [2.0, -1.0, 0.5, 0.75]], np.float32)
    times = np.array([0.0, np.nan, 1.0], np.float32)
    xi = np.array([1.0, 0.0, 0.0, 0.0, 0.0, 0.1])
    for fn in (DR.deskew, DR.deskew_f32):
        out = fn(pts, times, xi, 0.5)
        assert np.array_equal(out[1], [0.0, 0.0, 0.0, 0.25]) and not np.array_equal(out[0, :3], pts[0, :3])
        assert np.array_equal(fn(pts, times, np.zeros(6), 0.5), pts)
        assert np.array_equal(fn(pts, times, [0, 0, np.nan, 0, 0, 0], 0.5), pts)


def _cases():
    """(points, times, twist) of the GPU test's twists, for the float32 restatement."""
    g = np.random.default_rng(11)
    unit = lambda v: np.asarray(v, np.float64) / np.linalg.norm(v)
    twists = [[2.0, -1.0, 0.3, 0, 0, 0], [0, 0, 0, 0.1, -0.2, 0.3], np.concatenate([[1.5, 0.5, -0.2], 0.37 * unit([1, 2, 3])]),
              np.concatenate([[1.0, 1.0, 0.1], 1e-9 * unit([0, 0, 1])]), np.concatenate([[0.8, -0.4, 0.0], 0.9 * DR.SERIES_BELOW_F32 / 0.8 * unit([1, -1, 2])]),
              np.concatenate([[0.8, -0.4, 0.0], 1.1 * DR.SERIES_BELOW_F32 / 0.8 * unit([1, -1, 2])])]
    for xi in twists:
        n = 400
        p = np.concatenate([g.uniform(-40, 40, (n, 3)), g.uniform(0, 1, (n, 1))], 1).astype(np.float32)
        s = g.uniform(-0.2, 1.3, n).astype(np.float32)
        s[:4] = [0.0, 1.0, -0.2, 1.3]
        yield p, s, np.asarray(xi, np.float64)


def test_float32_restatement_stays_within_the_counted_bound():
    """The header's float32 sequence (with NumPy's sine, within 1 ulp) against the float64 reference: k 2^-24 (|p| + |tau||v|) per
    coordinate with k = kernel_k(0.5) = 17.3 -- the bound tests/test_gpu_deskew.py holds the kernel to."""
    k = DR.kernel_k(0.5)
    assert 17.0 < k < 18.0
    worst = 0.0
    for p, s, xi in _cases():
        scale, angle = DR.bound_scale(p, s, xi, 0.5)
        assert angle.max() <= 0.5
        err = np.abs(DR.deskew_f32(p, s, xi, 0.5).astype(np.float64) - DR.deskew(p, s, xi, 0.5))[:, :3].max(axis=1)
        worst = max(worst, float((err / (k * DR.U * scale)).max()))
    print("float32 restatement: largest error / bound = %.3f" % worst)
    assert worst <= 1.0


def test_azimuth_times():
    pts = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [-1, 1e-9, 0, 0], [0, -1, 0, 0]], np.float64)      # yaw 0, -90, -180, +90 degrees
    assert np.allclose(DR.azimuth_times(pts, -180.0, True), [0.5, 0.25, 0.0, 0.75], atol=1e-9)
    assert np.allclose(DR.azimuth_times(pts, -180.0, False)[[0, 1, 3]], [0.5, 0.75, 0.25], atol=1e-9)
    assert np.allclose(DR.azimuth_times(pts, 90.0, True), [0.75, 0.5, 0.25, 0.0], atol=1e-9)


# ---- refusals at the Python level -----------------------------------------------------------------------------------------------------
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
    """Stands in for the CDLL: ovn_deskew checks its arguments against EXT_SIGNATURES as ctypes would, notes the call, returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name not in _lib.EXT_SIGNATURES:
            raise AttributeError(name)
        res, argtypes = _lib.EXT_SIGNATURES[name]

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


TOOL_ARGS = {"odometry": ["--config", "c", "--scans", "s", "--out", "o"],
             "build_mesh": ["--config", "c", "--scans", "s", "--poses", "p", "--out", "o"],
             "slam": ["--config", "c", "--scans", "s", "--out", "o", "--overlap-thres", "none", "--min-fitness", "none", "--max-rms", "none",
                      "--odom-sigma", "1", "1", "--loop-sigma", "1", "1", "--huber", "none"]}


@pytest.mark.parametrize("tool", sorted(TOOL_ARGS))
@pytest.mark.parametrize("extra, message", [
    (["--deskew"], "needs a time source"),
    (["--deskew", "--start-azimuth", "10"], "come together"),
    (["--deskew", "--clockwise"], "come together"),
    (["--deskew", "--times", "d", "--start-azimuth", "0", "--clockwise"], "two time sources"),
    (["--times", "d"], "belong to --deskew"),
    (["--deskew", "--start-azimuth", "0", "--clockwise", "--counter-clockwise"], "not allowed with"),
], ids=["no-source", "no-direction", "no-start", "two-sources", "no-deskew", "both-directions"])
def test_tools_refuse_deskew_without_one_time_source(tool, extra, message, capsys):
    import importlib
    mod = importlib.import_module("tools." + tool)
    with pytest.raises(SystemExit) as stop:
        mod.main(TOOL_ARGS[tool] + extra)
    assert stop.value.code == 2 and message in capsys.readouterr().err          # argparse's own error, before any file is opened


def test_odometry_tool_refuses_other_passes(capsys):
    from tools import odometry as tool
    with pytest.raises(SystemExit) as stop:
        tool.main(TOOL_ARGS["odometry"] + ["--deskew", "--times", "d", "--deskew-passes", "3"])
    assert stop.value.code == 2 and "--deskew-passes" in capsys.readouterr().err


def test_config_refusals():
    assert D.check_config(None) is None
    assert D.check_config({}) == dict(t_ref=0.5, start_azimuth=None, clockwise=None)
    assert D.check_config(dict(t_ref=0.25, start_azimuth=180, clockwise=0)) == dict(t_ref=0.25, start_azimuth=180.0, clockwise=False)
    for bad in (dict(start_azimuth=0.0), dict(clockwise=True), dict(t_ref=float("nan")), dict(t_ref=1e60), dict(tref=0.5), True,
                dict(start_azimuth=float("inf"), clockwise=True), dict(start_azimuth=0.0, clockwise=2)):
        with pytest.raises(ValueError):
            D.check_config(bad)


def test_tracker_refusals():
    """On an engine that would fail at the first native call: the refusals come before it."""
    from overlapnet_amd import odometry
    eng = _fake_engine(object())
    box = dict(lo=[-2, -2, -1], hi=[2, 2, 1], voxel=0.5, proj_h=4, proj_w=8)
    for passes in (0, 3, 1.5, None):
        with pytest.raises(ValueError, match="deskew_passes"):
            odometry.TsdfOdometry(eng, deskew={}, deskew_passes=passes, **box)
    with pytest.raises(ValueError, match="deskew_passes"):
        odometry.RollingTsdfOdometry(eng, extent=(40.0, 40.0, 8.0), voxel=0.5, max_range=5.0, deskew={}, deskew_passes=3)
    with pytest.raises(ValueError, match="come together"):
        odometry.TsdfOdometry(eng, deskew=dict(clockwise=True), **box)
    pts = np.ones((5, 4), np.float32)
    odo = odometry.TsdfOdometry(eng, deskew={}, **box)
    with pytest.raises(ValueError, match="time source"):                 # azimuth parameters missing and no times
        odo.track(pts)
    for times in (np.zeros(4, np.float32), np.zeros((5, 1), np.float32)):
        with pytest.raises(ValueError, match="one fraction per point"):
            odo.track(pts, times=times)
    with pytest.raises(ValueError, match="deskew="):
        odometry.TsdfOdometry(eng, **box).track(pts, times=np.zeros(5, np.float32))
    offsets = np.array([0, 5], np.int64)
    with pytest.raises(ValueError, match="one fraction per point"):
        odometry.estimate_poses(eng, pts, offsets, deskew={}, times=np.zeros(6, np.float32))
    with pytest.raises(ValueError, match="deskew="):
        odometry.estimate_poses(eng, pts, offsets, times=np.zeros(5, np.float32))


def test_volume_refusals():
    from overlapnet_amd import tsdf
    eng = _fake_engine(object())
    vol = tsdf.TsdfVolume(eng, [-2, -2, -1], [2, 2, 1], 0.5)
    pts, offsets, poses = np.ones((5, 4), np.float32), np.array([0, 5], np.int64), np.eye(4)[None]
    with pytest.raises(ValueError, match="time source"):
        vol.integrate_scans(pts, offsets, poses, deskew={})
    with pytest.raises(ValueError, match="one fraction per point"):
        vol.integrate_scans(pts, offsets, poses, deskew={}, times=np.zeros(4, np.float32))
    with pytest.raises(ValueError, match="deskew="):
        vol.integrate_scans(pts, offsets, poses, twists=np.zeros((1, 6)))
    with pytest.raises(ValueError, match=r"twists must be \(1,6\)"):
        vol.integrate_scans(pts, offsets, poses, deskew={}, times=np.zeros(5, np.float32), twists=np.zeros((2, 6)))
    assert vol.n_scans == 0


def test_read_times_checks_every_scan(tmp_path):
    np.save(str(tmp_path / "000000.npy"), np.linspace(0, 1, 5).astype(np.float32))
    np.linspace(0, 1, 7).astype(np.float32).tofile(str(tmp_path / "000001.bin"))
    got = D.read_times(str(tmp_path), ["a/000000.bin", "a/000001.bin"], [5, 7])
    assert got.dtype == np.float32 and got.shape == (12,) and got[4] == 1.0 and got[5] == 0.0
    with pytest.raises(ValueError, match="a scan of 6 points"):
        D.read_times(str(tmp_path), ["a/000000.bin", "a/000001.bin"], [5, 6])
    with pytest.raises(ValueError, match="no times for scan 000002"):
        D.read_times(str(tmp_path), ["a/000002.bin"], [5])


# ---- the ledger of include/ovn_hip_deskew.h -------------------------------------------------------------------------------------------
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


def test_library_exports_the_extension_header():
    _lib.build()
    lib = C.CDLL(_lib.LIB_PATH)
    names = sorted(set(re.findall(r"\b(ovn_[a-z0-9_]+)\s*\(", _header_text())))
    assert names == ["ovn_deskew"]
    for n in names:
        assert hasattr(lib, n), "libovn_hip.so does not export %s declared in include/ovn_hip_deskew.h" % n
    assert sorted(_lib.EXT_SIGNATURES) == names
    assert '#include "ovn_hip.h"' in open(HEADER).read()
    bound = _lib.load()                                       # load() binds the extension table in the same loop
    assert bound.ovn_deskew.argtypes == _lib.EXT_SIGNATURES["ovn_deskew"][1] and bound.ovn_deskew.restype is C.c_int


def test_ext_signatures_have_the_types_of_the_header():
    protos = _header_prototypes()
    assert sorted(protos) == sorted(_lib.EXT_SIGNATURES) and not set(_lib.EXT_SIGNATURES) & set(_lib.SIGNATURES)
    wrong = []
    for name, (ret, params) in protos.items():
        res, args = _lib.EXT_SIGNATURES[name]
        if res is not _SCALARS[ret]:
            wrong.append("%s returns %s, EXT_SIGNATURES says %s" % (name, ret, res.__name__))
        if len(args) != len(params):
            wrong.append("%s takes %d parameters, EXT_SIGNATURES lists %d" % (name, len(params), len(args)))
            continue
        for i, ((c, _), a) in enumerate(zip(params, args)):
            if not any(a is ok for ok in _ctypes_accepted(c)):
                wrong.append("%s parameter %d is %s, EXT_SIGNATURES says %s" % (name, i, c, a.__name__))
    assert not wrong, "\n".join(wrong)
    assert [n for _, n in protos["ovn_deskew"][1]][:2] == ["ctx", "stream"]          # the stream comes second, as the header says


def test_a_missing_extension_symbol_is_the_usual_error(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.EXT_SIGNATURES, "ovn_no_such_call", (C.c_int, []))
    with pytest.raises(_lib.OvnError, match="does not export ovn_no_such_call"):
        _lib.load()


def test_argument_errors_of_the_library_without_a_gpu():
    lib = _lib.load()
    assert lib.ovn_deskew(None, None, None, None, 1, None, 0.0, 0, None, 0.5, None) == 1 and b"ctx is NULL" in lib.ovn_last_error()


def _inputs(n_scans=2, total=7):
    return dict(points=torch.rand(total, 4), offsets=torch.tensor([0, 3, total][:n_scans + 1], dtype=torch.int64),
                twists=torch.rand(n_scans, 6, dtype=torch.float64), times=torch.rand(total))


def test_deskew_scans_passes_the_header_arguments_in_order():
    rec = Recorder()
    eng = _fake_engine(rec)
    a = _inputs()
    out = D.deskew_scans(eng, a["points"], a["offsets"], a["twists"], times=a["times"], t_ref=0.25)
    again = D.deskew_scans(eng, a["points"], a["offsets"], a["twists"].numpy(), start_azimuth=-180.0, clockwise=True, out=a["points"])
    assert out.shape == (7, 4) and out.dtype == torch.float32 and out.data_ptr() != a["points"].data_ptr() and again is a["points"]
    names = [n for _, n in _header_prototypes()["ovn_deskew"][1]]
    assert names == ["ctx", "stream", "points_dev", "offsets_dev", "n_scans", "times_dev", "start_azimuth_deg", "clockwise", "twists_dev",
                     "t_ref", "out_points_dev"]
    value = lambda v: getattr(v, "value", v)
    first = dict(zip(names, (value(v) for v in rec.calls[0][1])))
    assert first == dict(ctx=HANDLE, stream=STREAM, points_dev=a["points"].data_ptr(), offsets_dev=a["offsets"].data_ptr(), n_scans=2,
                         times_dev=a["times"].data_ptr(), start_azimuth_deg=0.0, clockwise=0, twists_dev=a["twists"].data_ptr(), t_ref=0.25,
                         out_points_dev=out.data_ptr())
    second = dict(zip(names, (value(v) for v in rec.calls[1][1])))
    assert second["times_dev"] is None and second["start_azimuth_deg"] == -180.0 and second["clockwise"] == 1 and second["t_ref"] == 0.5
    assert second["out_points_dev"] == second["points_dev"] == a["points"].data_ptr() and len(rec.calls) == 2


@pytest.mark.parametrize("arg", ["points", "offsets", "twists", "times", "out"])
@pytest.mark.parametrize("kind", ["dtype", "device", "contiguity", "shape"])
def test_deskew_scans_refuses_bad_tensors_before_the_library(arg, kind):
    rec = Recorder()
    eng = _fake_engine(rec)
    a = _inputs()
    a["out"] = torch.empty(7, 4)
    t = a[arg]
    if kind == "dtype":
        bad = t.to(torch.float64 if t.dtype != torch.float64 else torch.float32)
    elif kind == "device":
        bad = t.to("meta")
    elif kind == "contiguity":
        wide = torch.zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],), dtype=t.dtype)
        bad = wide[..., ::2]
        assert not bad.is_contiguous() and bad.shape == t.shape
    else:
        bad = torch.zeros((t.shape[0] + 1,) + tuple(t.shape[1:]), dtype=t.dtype) if arg != "points" else torch.rand(7, 3)
    a[arg] = bad
    with pytest.raises(_lib.OvnError):
        D.deskew_scans(eng, a["points"], a["offsets"], a["twists"], times=a["times"], out=a["out"])
    assert rec.calls == []


def test_deskew_scans_refuses_a_missing_time_source_and_partial_overlap():
    rec = Recorder()
    eng = _fake_engine(rec)
    a = _inputs()
    for kw in (dict(), dict(start_azimuth=0.0), dict(clockwise=True), dict(times=a["times"], start_azimuth=0.0, clockwise=True),
               dict(start_azimuth=float("nan"), clockwise=True), dict(start_azimuth=0.0, clockwise=3), dict(times=a["times"], t_ref=float("inf"))):
        with pytest.raises(ValueError):
            D.deskew_scans(eng, a["points"], a["offsets"], a["twists"], **kw)
    big = torch.rand(9, 4)
    with pytest.raises(_lib.OvnError, match="overlaps"):
        D.deskew_scans(eng, big[:7], a["offsets"], a["twists"], times=a["times"], out=big[2:])
    assert rec.calls == []
