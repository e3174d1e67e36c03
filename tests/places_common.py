"""What the place-recognition tests share: the drive whose sweeps are stored and queried on the GPU (test_gpu_places.py) and checked on
the model alone (test_places_model.py), and the NaN / range filter of scan registration for the model-only tests."""
import numpy as np

# The batch of the GPU match tests: slot b registers sweep b of this drive; the even slots are stored, the odd slots are the queries.
MATCH_DRIVE = dict(name="HDL-64", frames=24, seed=7, columns=512, travel=True, step=1.6)
MATCH_T = 4


def db_slots():
    return list(range(0, MATCH_DRIVE["frames"], 2))


def query_slots():
    return list(range(1, MATCH_DRIVE["frames"], 2))


def kept(scan, min_range):
    """The points that pass NaN removal + removeClosedPointCloud (float32 arithmetic).  ALOAM_CLOUD_FULL is a subset of them: scan
    registration also drops the rays whose elevation maps to no ring (src/scanRegistration.cpp:166-205).  Good enough for the model-only tests;
    the GPU tests take the descriptor's input from the device's own full cloud."""
    p = np.asarray(scan, np.float32)[:, :3]
    ok = np.isfinite(p).all(axis=1)
    r2 = p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2]
    thr = np.float32(min_range) * np.float32(min_range)
    with np.errstate(invalid="ignore"):
        ok &= ~(r2 < thr)
    return p[ok]
