"""The numpy model of aloam_graph_register_loops (a-loam_amd/loopreg.py, tests/loopreg_model.py), no GPU: the rotation of the information into
the edge's tangent against central differences, the target of one node, and the fixture the GPU tests register."""
import importlib
import math

import numpy as np
import pytest

import loopreg_model as M


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("a-loam_amd.loopreg")


@pytest.fixture(scope="module")
def P():
    return importlib.import_module("a-loam_amd.posegraph")


def test_edge_information_against_central_differences_of_the_registration_cost(L, P):
    """Factor records that Z satisfies exactly (f64 points on their lines and planes): the cost along the graph's residual,
    Z' = Z o (exp(h phi / 2), h tau), is 1/2 h^2 xi^T info xi up to h^4, the cubic term cancelling between +h and -h.  Z is rotated by
    0.9 rad about a tilted axis, so a dropped or transposed T = blockdiag(R_Z, R_Z) changes every block.  Step and bound are those of
    test_gradient_against_central_differences: h = 1e-6, 1e-7 relative (h^2 truncation plus the rounding of residuals of size h)."""
    information = importlib.import_module("a-loam_amd.information")
    rng = np.random.default_rng(5)
    axis = np.array([0.3, -0.5, 0.8]); axis /= np.linalg.norm(axis)
    qz, tz = P.qexp(0.9 * axis), np.array([1.5, -0.7, 0.4])
    n_l, n_p = 40, 120
    w = rng.uniform(-8, 8, (n_l, 3)); d = rng.normal(size=(n_l, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
    on = w + rng.uniform(-0.5, 0.5, (n_l, 1)) * d                                 # a point of every line, and its sensor-frame twin
    qi, ti = P.inverse(qz, tz)
    lines = np.concatenate([P.qrot(qi, on) + ti, w + 0.1 * d, w - 0.1 * d], 1)
    n = rng.normal(size=(n_p, 3)); n[:, 2] *= 0.2; n /= np.linalg.norm(n, axis=1)[:, None]   # mostly walls: an anisotropic information
    pw = rng.uniform(-8, 8, (n_p, 3))
    planes = np.concatenate([P.qrot(qi, pw) + ti, n, -np.einsum("ij,ij->i", n, pw)[:, None]], 1)
    rec = information.information_from_factors(lines, planes, qz, tz)
    assert rec["cost"] < 1e-25
    info = L.edge_information(rec["info"], qz)
    assert np.array_equal(L.edge_information(P.info_upper(rec["info"]), qz), P.info_upper(info))
    h = 1e-6

    def quad(xi):
        c = 0.0
        for sgn in (1.0, -1.0):
            q1 = P.qmul(qz, P.qexp(sgn * h * xi[:3]))
            t1 = tz + P.qrot(qz, sgn * h * xi[3:])
            c += information.information_from_factors(lines, planes, q1, t1)["cost"]
        return (c - 2.0 * rec["cost"]) / (h * h)                                     # = xi^T info xi

    E = np.eye(6)
    diag = np.array([quad(E[a]) for a in range(6)])
    num = np.diag(diag)
    for a in range(6):
        for b in range(a + 1, 6):
            num[a, b] = num[b, a] = 0.5 * (quad(E[a] + E[b]) - diag[a] - diag[b])
    err = np.abs(num - info).max() / np.abs(info).max()
    left = np.abs(num - rec["info"]).max() / np.abs(info).max()
    R = P.rotmat(qz)
    T = np.zeros((6, 6)); T[:3, :3] = R; T[3:, 3:] = R
    transposed = np.abs(num - T @ rec["info"] @ T.T).max() / np.abs(info).max()
    print(f"edge information against central differences: relative {err:.3e}; left-tangent matrix unchanged {left:.3e}, T transposed {transposed:.3e}")
    assert err <= 1e-7
    assert left > 1e-2 and transposed > 1e-2                                         # the check tells the three apart


def test_target_of_one_node_at_the_identity_is_the_filter_of_its_cloud(L, O):
    rng = np.random.default_rng(3)
    c, f = M.world_sample(rng, 300, 1500)
    clouds = [(M.sensor_cloud(c, (0, 0, 0, 1), (0, 0, 0), rng), M.sensor_cloud(f, (0, 0, 0, 1), (0, 0, 0), rng))]
    tc, ts = L.target_cloud(np.array([[0.0, 0.0, 0.0, 1.0]]), np.zeros((1, 3)), clouds, 0, 0, 1, M.LEAF, M.voxel_filter)
    for got, raw, leaf in ((tc, clouds[0][0], M.LEAF[0]), (ts, clouds[0][1], M.LEAF[1])):
        want = O.voxel_filter(raw, leaf, canonical=True)
        assert len(want) > 50 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_the_model_registers_the_fixture(L, P):
    """The fixture of the GPU tests (nine target nodes along 8 m, a source whose entered pose is off by about 0.4 m and 4 degrees): the
    model alone ends at no more than a tenth of the guess's error, in rotation and in translation.  A condition on the inputs."""
    fx = M.fixture()
    clouds = M.keyframe_clouds(fx)
    sizes = np.array([[len(c), len(f)] for c, f in clouds])
    print("keyframe clouds (corner, surf): min", sizes.min(0), "max", sizes.max(0))
    tc, ts = L.target_cloud(fx["q"], fx["t"], clouds, fx["i"], fx["first"], fx["count"], M.LEAF, M.voxel_filter)
    (qg, tg), (qt, tt) = M.request_of(fx)
    r0, d0 = M.pose_error(qg, tg, qt, tt)
    assert 0.35 < d0 < 0.5 and math.radians(3.5) < r0 < math.radians(4.5)
    res = M.register(tc, ts, clouds[fx["j"]][0], clouds[fx["j"]][1], qg, tg)
    r1, d1 = M.pose_error(res["q"], res["t"], qt, tt)
    print(f"model registration: target {len(tc)} + {len(ts)} points, factors {res['n_line']} + {res['n_plane']}, LM {res['lm_iterations']} termination "
          f"{res['lm_termination']}; rotation {r0:.4f} -> {r1:.2e} rad (ratio {r1 / r0:.2e}), translation {d0:.4f} -> {d1:.2e} m (ratio {d1 / d0:.2e})")
    assert res["status"] == L.LOOP_OK
    assert r1 <= 0.1 * r0 and d1 <= 0.1 * d0
    w = np.linalg.eigvalsh(res["info"])
    assert w[0] > 0 and np.allclose(np.sort(np.linalg.eigvalsh(res["info_left"])), w, rtol=1e-9)      # a congruence by a rotation keeps the spectrum
