import atexit
import shutil
"""GPU-box helper: where the merged tracker's time goes on the 20 x 40 synthetic split (after one chain run has produced `merged`).
    python tools/profile_tracker.py
    python tools/profile_tracker.py --hungarian    # hungarian=True: host solver per frame / device solver per frame / whole scenes"""
import cProfile
import gc
import os
import pstats
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shasta_amd import pipeline, pub_tracker, scenes  # noqa: E402


def main():
    dev = torch.device("cuda", 0)
    root = tempfile.mkdtemp(prefix="shasta_split_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    atexit.register(shutil.rmtree, root, ignore_errors=True)  # the split lives in RAM (tmpfs): never leave it behind
    paths, sc = scenes.write_synthetic_split(root, n_scenes=20, frames_per_scene=40, seed=3)
    models = {n: pipeline.build_class_model(n, dev, seed=1) for n in pipeline.CLASS_CONFIGS}
    _, merged, _ = pipeline.run_split(models, paths, sc, scenes.TokenNeck(), dev, batch_pairs=40)
    import json
    meta = json.load(open(paths["frames_meta_path"]))["frames"]
    gc.disable()
    acc = {"prepare": 0.0, "device": 0.0, "finish": 0.0}
    orig_prepare, orig_dev, orig_fin = pub_tracker.PubTrackerMerged._prepare, pub_tracker.center_greedy_device, pub_tracker.PubTrackerMerged._finish_class

    def timed(name, fn):
        def w(*a, **k):
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                acc[name] += time.perf_counter() - t0
        return w
    pub_tracker.PubTrackerMerged._prepare = timed("prepare", orig_prepare)
    pub_tracker.center_greedy_device = timed("device", orig_dev)
    pub_tracker.PubTrackerMerged._finish_class = timed("finish", orig_fin)
    # --hungarian: the three routes of hungarian=True.  LSAP_CAP = 0 sends every problem down the over-capacity route, which is the
    # route every problem took before the device solver: float64 matrices back to the host, scipy per problem
    cap = pub_tracker.LSAP_CAP
    modes = [("tracker", {}, cap)]
    if "--hungarian" in sys.argv:
        modes = [("hungarian, per frame, scipy on the host", dict(hungarian=True), 0), ("hungarian, per frame, device solver", dict(hungarian=True), cap),
                 ("hungarian, whole scenes in one launch", dict(hungarian=True, whole_scenes=True), cap)]
    want = None
    for rep in range(5 if len(modes) > 1 else 3):  # the routes take turns: a difference has to show in every round (the first is warm-up)
        for name, kw, lsap_cap in modes:
            pub_tracker.LSAP_CAP = lsap_cap
            for k in acc:
                acc[k] = 0.0
            preds = {tok: [dict(d) for d in annos] for tok, annos in merged["results"].items()}
            t0 = time.perf_counter()
            got = pipeline.run_tracking(preds, meta, max_age=4, **kw)
            total = time.perf_counter() - t0
            print("%s %.3f s: " % (name, total) + ", ".join("%s %.3f" % kv for kv in acc.items()) + ", rest %.3f" % (total - sum(acc.values())), flush=True)
            want = want or got
            assert got == want, "the routes disagree"


if __name__ == "__main__":
    main()
