"""Pin of the neural path on the ONLY result the reference publishes: the title of `pics/demo2.png`, "Overlap: [0.8919191]  Yaw: [0]",
produced by demo2 with the authors' trained `model_geo.weight` (README.md:120 of the reference gives a download link; the file is
git-ignored upstream, .gitignore:9, and is not in this tree, so no test can run this -- run it by hand once the file is at hand):

    python tools/demo2_published.py /path/to/model_geo.weight          (needs an MI355X; exit status 0 = both modes within tolerance)

It follows demo1 + demo2 step by step:
  * demo1 (demo1_gen_data.py -> gen_depth_data.py:10-48, gen_normal_data.py:10-46): the two shipped scans data/scans/00000{0,1}.bin
    (embedded in tests/golden/kitti_preprocess.npz) -> depth/ and normal/ .npy files of sequence "preprocess_data_demo";
  * demo2 (demo2_infer.py:52-69): config/network.yml as shipped (depth + normals, 360OutputkLegs, DeltaLayerConv1NetworkHead,
    CorrelationHead), `infer_seqs = Demo2.infer_seqs`, and -- note the swap at demo2_infer.py:69 --
    `Infer(config).infer_one(scan2_path, scan1_path)`; inside, infer.py:138-152 makes scan1 the LEFT input of the head.
The check is north_star's tolerance: |overlap - 0.8919191| <= 1e-4 and yaw == 0, in the default (f16x3) and the fp32 mode.
tests/test_demo2_published.py runs the same flow (`run_demo2`) on a seeded full-size weight file against the fp64 oracle."""
import os
import pathlib
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PUBLISHED_OVERLAP = 0.8919191     # pics/demo2.png
PUBLISHED_YAW = 0


def network_yml(data_root, weightfile):
    """config/network.yml of the reference, as a dict (the keys `Infer` reads: infer.py:31-93,117)."""
    return {"pretrained_weightsfilename": weightfile,
            "use_depth": True, "use_normals": True, "use_class_probabilities": False, "use_class_probabilities_pca": False,
            "use_intensity": False, "data_root_folder": str(data_root), "infer_seqs": "preprocess_data_demo", "batch_size": 16,
            "model": {"modelType": "SiameseNetworkTemplate", "legsType": "360OutputkLegs",
                      "overlap_head": "DeltaLayerConv1NetworkHead", "orientation_head": "CorrelationHead",
                      "inputShape": [64, 900], "leg_output_width": 360, "strides_layer1": [2, 2],
                      "additional_unsymmetric_layer3a": True}}


def run_demo2(work_dir, fx, weightfile, precision=None):
    """demo1 on the two shipped scans, then demo2, under `work_dir` (a pathlib.Path); returns (Infer, overlap, yaw)."""
    from overlapnet_amd import preprocess as P
    from overlapnet_amd.infer import Infer
    scans = work_dir / "data" / "scans"
    os.makedirs(scans)
    fx["points_0"].astype(np.float32).tofile(scans / "000000.bin")
    fx["points_1"].astype(np.float32).tofile(scans / "000001.bin")
    dst = work_dir / "data" / "preprocess_data_demo"
    os.makedirs(dst)
    P.gen_depth_data(str(scans), str(dst))        # demo1
    P.gen_normal_data(str(scans), str(dst))
    cfg = network_yml(work_dir / "data", weightfile)
    if precision:
        cfg["precision"] = precision              # extension key of this framework: every contraction on the fp32 matrix cores
    infer = Infer(cfg)
    scan1_path, scan2_path = str(scans / "000000.bin"), str(scans / "000001.bin")
    overlap, yaw = infer.infer_one(scan2_path, scan1_path)        # demo2_infer.py:69 passes (scan2, scan1)
    assert list(infer.filenames) == ["000000", "000001"]          # infer.py:148: [name2, name1] -> what demo2 plots as scan1, scan2
    assert overlap.shape == (1,) and yaw.shape == (1,)
    return infer, overlap, yaw


def main(argv):
    if len(argv) != 1 or not os.path.isfile(argv[0]):
        raise SystemExit("usage: python tools/demo2_published.py /path/to/model_geo.weight")
    from tools import synthetic as S
    fx = S.load_fixture_images()
    ok = True
    for precision in (None, "f32"):
        with tempfile.TemporaryDirectory() as d:
            _, overlap, yaw = run_demo2(pathlib.Path(d), fx, argv[0], precision)
        good = abs(float(overlap[0]) - PUBLISHED_OVERLAP) <= 1e-4 and int(yaw[0]) == PUBLISHED_YAW
        ok = ok and good
        print("demo2 [%s]: overlap %r yaw %r (published: [%s] [%d]) %s"
              % (precision or "default", overlap, yaw, PUBLISHED_OVERLAP, PUBLISHED_YAW, "ok" if good else "DIFFERS"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
