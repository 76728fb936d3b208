"""CPU: every entry point of include/ovn_hip.h that takes a `stream` has a row in the stream-contract table.

tests/test_gpu_stream_contract.py calls each route of the library on a non-default stream; what it covers is its table ROWS.  This file
reads the header's prototypes and holds the table against them, so that an entry point added later without a stream test fails here,
on a machine without a GPU."""
import os
import re

from tests import test_gpu_stream_contract as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_EXEMPT = 6


def _stream_prototypes():
    """Names of the header's functions whose parameter list ends in `void* stream)`."""
    with open(os.path.join(ROOT, "include", "ovn_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)                    # comments name functions too
    protos = re.findall(r"\b(?:int|int64_t|const char\*)\s+(ovn_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)
    assert len(protos) >= 60, "the header's prototypes were not all found (%d)" % len(protos)
    return [name for name, params in protos if re.search(r"void\s*\*\s*stream\s*$", params.strip())]


def test_the_header_parser_finds_the_known_entry_points():
    names = _stream_prototypes()
    assert len(names) == len(set(names)) and len(names) >= 39
    for known in ("ovn_leg", "ovn_heads_spectral", "ovn_heads_segments", "ovn_render_scans", "ovn_tsdf_triangles", "ovn_mcl_resample",
                  "ovn_icp_register", "ovn_head_walk_stats", "ovn_gather_scores", "ovn_add_leg_layer"):
        assert known in names
    for streamless in ("ovn_create", "ovn_finalize", "ovn_set_head_pipeline", "ovn_profile_end", "ovn_selftest", "ovn_comm_init"):
        assert streamless not in names


def test_every_entry_point_with_a_stream_has_a_row():
    names = _stream_prototypes()
    covered = {f for r in T.ROWS for f in r.covers}
    missing = [n for n in names if n not in covered and n not in T.EXEMPT]
    assert not missing, "no row of tests/test_gpu_stream_contract.py calls %s on a non-default stream" % missing
    unknown = sorted((covered | set(T.EXEMPT)) - set(names))
    assert not unknown, "rows or exemptions name functions the header does not declare with a stream: %s" % unknown
    both = sorted(covered & set(T.EXEMPT))
    assert not both, "exempt and covered at once: %s" % both


def test_rows_are_well_formed():
    assert len({r.name for r in T.ROWS}) == len(T.ROWS), "row names repeat"
    for r in T.ROWS:
        assert r.covers and callable(r.build), r.name
        assert r.klass in (T.ENQUEUE_ONLY, T.SYNCHRONISES), r.name
        if r.klass == T.SYNCHRONISES:
            assert isinstance(r.reason, str) and len(r.reason.strip()) >= 20, "%s is classed `synchronises` without a reason" % r.name
        else:
            assert r.reason is None, "%s: a reason belongs to a `synchronises` row" % r.name


def test_synchronising_rows_quote_text_that_exists():
    """The quoted part of a reason stands, word for word, in the header or in the wrapper."""
    with open(os.path.join(ROOT, "include", "ovn_hip.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "overlapnet_amd", "engine.py")) as f:
        engine = f.read()
    flat = lambda s: re.sub(r"[\s*]+", " ", s)
    sources = flat(header) + flat(engine)
    for r in T.ROWS:
        if r.klass != T.SYNCHRONISES:
            continue
        quotes = re.findall(r"\"([^\"]+)\"", r.reason)
        assert quotes, "%s: the reason quotes nothing" % r.name
        for q in quotes:
            assert flat(q) in sources, "%s: %r is neither in include/ovn_hip.h nor in overlapnet_amd/engine.py" % (r.name, q)


def test_exemptions_are_few_and_reasoned():
    assert len(T.EXEMPT) <= MAX_EXEMPT
    for name, reason in T.EXEMPT.items():
        assert isinstance(reason, str) and len(reason.strip()) >= 20 and "\n" not in reason, name


def test_the_named_rows_of_the_other_tests_exist():
    names = {r.name for r in T.ROWS}
    for n in ("spectrum", "heads_spectra_dcache", "project", "heads_segments", "leg_f16x3", "top_k", "mcl_update"):
        assert n in names
