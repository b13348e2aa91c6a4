"""Generates tests/golden/association_golden.json: seeded detection / track boxes and what the REFERENCE's
mot_3d.association.associate_dets_to_tracks (imported in place; build container only) returns for them, for the greedy and
bipartite matchers under the euler and m_dis distances.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_association_golden.py
"""
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import as R  # noqa: E402

SCALE = [5, 5, 1, 3, 1, 1, 1]  # the 7-vector [x, y, z, o, l, w, h] of BBox.array2bbox


def cases():
    """The inputs, drawn in the order tests/test_host_logic.py drew them when it imported the reference directly."""
    rng = np.random.default_rng(2)
    for mode in ("greedy", "bipartite"):
        for asso in ("euler", "m_dis"):
            dets = [rng.normal(size=7) * SCALE for _ in range(7)]
            trks = [rng.normal(size=7) * SCALE for _ in range(5)]
            inn = [np.eye(7) * rng.uniform(0.5, 2) + 0.1 for _ in trks] if asso == "m_dis" else None
            yield mode, asso, dets, trks, inn


def main():
    ref = R.import_association()
    from mot_3d.data_protos import BBox
    out = []
    for mode, asso, dets, trks, inn in cases():
        m, ud, ut = ref.associate_dets_to_tracks([BBox.array2bbox(d) for d in dets], [BBox.array2bbox(t) for t in trks], mode, asso, 3.0, inn)
        out.append({"mode": mode, "asso": asso, "dist_threshold": 3.0,
                    "dets": [[float(v) for v in d] for d in dets], "trks": [[float(v) for v in t] for t in trks],
                    "innovation": None if inn is None else [np.asarray(x, np.float64).tolist() for x in inn],
                    "matches": [[int(v) for v in x] for x in m], "unmatched_dets": [int(v) for v in ud],
                    "unmatched_trks": [int(v) for v in ut]})
    path = os.path.join(HERE, "association_golden.json")
    with open(path, "w") as f:
        json.dump({"source": "mot_3d/association.py associate_dets_to_tracks of the reference", "cases": out}, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
