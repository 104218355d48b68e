"""Child process of tests/test_lidar.py: one lidar sweep of a model read from an .npz file (model, pose, and the sensor's fields), under
whatever SM_LIDAR_* switches the parent put into the environment; the four planes and the call's stats go into another .npz."""
import sys

import numpy as np


def main(src, dst):
    from surfelmapping_amd import capi
    a = np.load(src)
    m = capi.SurfelMap(capi.make_config(64, 48, 50.0, 50.0, 31.5, 23.5, max_sqrt_vertices=200))
    m.upload_model(np.ascontiguousarray(a["model"], np.float32))
    sn = capi.lidar_sensor(n_az=int(a["n_az"]), az0_deg=float(a["az0"]), az_step_deg=float(a["step"]), el_deg=a["el"],
                           min_range=float(a["min_range"]), max_range=float(a["max_range"]), min_conf=float(a["min_conf"]))
    out = m.lidar_sweep(a["pose"], sn)
    st = m.lidar_stats()
    np.savez(dst, **out, **{"stat_" + k: v for k, v in st.items()})
    m.close()


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
