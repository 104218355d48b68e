"""Child process of tests/test_points.py: one point query into a model read from an .npz file (model, points, cell_mm), under whatever
SM_POINTS_* switches the parent put into the environment; the planes and the call's stats go into another .npz."""
import sys

import numpy as np


def main(src, dst):
    from surfelmapping_amd import capi
    a = np.load(src)
    m = capi.SurfelMap(capi.make_config(64, 48, 50.0, 50.0, 31.5, 23.5, max_sqrt_vertices=200))
    m.upload_model(np.ascontiguousarray(a["model"], np.float32))
    out = m.query_points(a["points"], cell_mm=int(a["cell_mm"]))
    st = m.query_points_stats()
    np.savez(dst, **out, **{"stat_" + k: v for k, v in st.items()})
    m.close()


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
