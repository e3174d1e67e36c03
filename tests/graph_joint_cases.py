"""The constructed groups of the joined pose graphs (aloam_graph_optimize_joint), shared by the model's test and the GPU test.
Every builder is seeded and small."""
import numpy as np

import graph_trim_cases as tc
from posegraph_cases import pg

# The frame the second session of a cut drive is expressed in: a rotation by 2 rad and a translation by 100 m.
_AXIS, _DIR = np.array([0.3, -1.1, 2.0]), np.array([60.0, -70.0, 40.0])
FRAME = (pg.qexp(2.0 * _AXIS / np.linalg.norm(_AXIS)), 100.0 * _DIR / np.linalg.norm(_DIR))
CUTS = (((3, 120, 4), 70), ((5, 90, 3), 31), ((1, 300, 2), 140))


def random_links(seed, seq_i, i, seq_j, j, robust=None):
    """Links with unrelated measurements and dense information, about half of them flagged robust unless `robust` says otherwise."""
    i, j = np.atleast_1d(i), np.atleast_1d(j)
    e = tc.random_edges(seed, i, j, robust)
    return pg.make_links(seq_i, i, seq_j, j, e["q"], e["t"], pg.info_full(e["info"]), e["flags"] != 0)


def byte_group(middle, seqs=(0, 1, 2)):
    """Three members with 1, `middle` and 2 nodes for the bytes of gather, align and scatter.  Member 0: one node and one anchor on it.
    Member 1: `middle` nodes, its odometry edges and one or four more (255, 256 and 260 edges for 255, 256 and 257 nodes), anchors among them.  Member 2: two nodes, an
    odometry edge and an anchor.  Links in both directions; the first link listed joins members 0 and 1 with member 1 on the seq_i side,
    the second one is a second link between the same two (so the tree link of member 2 is not the first link listed), and member 2 hangs on
    member 1 (a chain of two aligned members) by a link that has it on the seq_j side, then on member 0.
    Returns (members [(q, t, extra edges)], links, the odometry information)."""
    a, b, c = seqs
    rng = np.random.default_rng(middle)
    sizes = (1, middle, 2)
    poses = [(tc.unit(rng.standard_normal((n, 4))), rng.uniform(-50, 50, (n, 3))) for n in sizes]
    n_extra = 4 if middle > 256 else 1                               # beside the middle - 1 odometry edges: 255, 256 and 260 edges for 255, 256 and 257 nodes
    i = rng.integers(-1, middle, n_extra)
    j = rng.integers(0, middle, n_extra)
    j = np.where(i == j, (j + 1) % middle, j)
    i[:4] = -1                                                        # anchors for certain
    extra = [tc.random_edges(10, [-1], [0], seq=a), tc.random_edges(11 + middle, i, j, seq=b), tc.random_edges(12, [-1, -1], [1, 0], seq=c)]
    links = np.concatenate([random_links(20, b, middle - 1, a, 0), random_links(21, a, 0, b, middle // 2),
                            random_links(22, b, 3 % middle, c, 1), random_links(23, c, 0, a, 0), random_links(24, a, 0, c, 1)])
    return [(poses[m][0], poses[m][1], extra[m]) for m in range(3)], links, np.eye(6) * 40.0


def own_residuals(nodes, edges):
    return pg.residual(nodes["q_opt"], nodes["t_opt"], edges)
