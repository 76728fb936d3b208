"""GPU: `Infer(config, rank=, world=2).infer_top_k` -- each rank ranks the references it owns on the device and one all-gather of
k x 16 B per rank carries the lists -- must give exactly the single-process lists over a streaming replay (two processes on cuda:0,
gloo rendezvous, as tests/test_gpu_two_ranks.py does), and a failure of one rank's local work must reach both."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_sharded_infer_top_k_equals_the_single_process_lists(tmp_path, fixture_npz):
    from tools import synthetic as S
    frames = 30
    seq = tmp_path / "data" / "07"
    for sub in ("depth", "normal"):
        os.makedirs(seq / sub)
    for i in range(frames):
        s, shift = i % 2, (37 * i) % 900
        np.save(seq / "depth" / ("%06d.npy" % i), np.roll(fixture_npz["range_%d" % s], shift, axis=1))
        np.save(seq / "normal" / ("%06d.npy" % i), np.roll(fixture_npz["normal_%d" % s], shift, axis=1))
    cfg = {"model": dict(S.REFERENCE_MODEL_CFG, inputShape=[64, 900]), "infer_seqs": "07", "data_root_folder": str(tmp_path / "data"),
           "use_depth": True, "use_normals": True, "use_class_probabilities": False, "use_class_probabilities_pca": False,
           "use_intensity": False, "batch_size": 16, "pretrained_weightsfilename": "", "_frames": frames}
    json.dump(cfg, open(tmp_path / "config.json", "w"))
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="4")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_top_k_two_rank_worker.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=600)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-3000:] for o in outs)
    r = json.load(open(tmp_path / "result.json"))
    assert r["calls"] == frames - 1 >= 20 and r["mismatch"] == [], r["mismatch"]
    assert sorted(set(r["ks"])) == [1, 5, 64] and r["nonempty"] >= 15, r
    assert all(s["pairs_scored"] > 100 for s in r["stats"]), r["stats"]          # both ranks scored their share
    f = r["one_rank_failure"]
    assert all("rank(s) [1]" in m for m in f[0]) and all("simulated" in m for m in f[1]), f
    assert r["retry_ok"] is True
