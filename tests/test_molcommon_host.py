"""CPU: the index arithmetic the six molecule kernels share (phoregen_amd/csrc/mol_common.h) compiled for the host under ASan / UBSan
(tools/mol_common_host_check.cpp): the lane-strided walk over a graph's pairs against numpy's row-major unranking, and the frame and
point-range guards against expectations written out here.

The kernels themselves are held against their restatements in tests/test_gpu_mol*.py."""
import os
import shutil

import numpy as np
import pytest

from mol_support import build_host_check, run_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_ATOMS = 128
pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='no g++ to compile the host check with')


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return build_host_check('mol_common_host_check', tmp_path_factory.mktemp('mol_common'))


def test_pair_walk_visits_its_lane_share_in_row_major_order(exe):
    out = run_program(exe, 'pairs', MAX_ATOMS)
    got = np.array(' '.join(out).split(), dtype=np.int64).reshape(-1, 5)                    # n, lane, p, a, b in the order visited
    want = []
    for n in range(MAX_ATOMS + 1):
        a, b = np.triu_indices(n, 1)                                             # row-major: pair p is (a[p], b[p])
        p = np.arange(n * (n - 1) // 2)
        assert np.array_equal(p, a * n - a * (a + 1) // 2 + (b - a - 1)) and bool(np.all((0 <= a) & (a < b) & (b < n)))
        order = np.lexsort((p, p % 64))                                          # by lane, increasing p inside a lane
        want.append(np.stack([np.full(p.size, n), p[order] % 64, p[order], a[order], b[order]], 1))
    want = np.concatenate(want)
    assert want.shape[0] == sum(n * (n - 1) // 2 for n in range(MAX_ATOMS + 1))
    assert got.shape == want.shape and np.array_equal(got, want)


def _pairs(n):
    return n * (n - 1) // 2


def _case(sizes, points, F=2, **over):
    """One batch: graph sizes and per-graph point counts (every graph its own points), and whatever a test overrides."""
    sizes, points = np.asarray(sizes), np.asarray(points)
    c = dict(F=F, B=len(sizes), n_lig=int(sizes.sum()), n_half=int(sum(_pairs(n) for n in sizes)), n_point=int(points.sum()),
             n_out=int(points.sum()), lig_off=np.concatenate([[0], np.cumsum(sizes)]),
             bond_off=np.concatenate([[0], np.cumsum([2 * _pairs(n) for n in sizes])]),
             out_off=np.concatenate([[0], np.cumsum(points)]))
    c['range'] = np.stack([c['out_off'][:-1], c['out_off'][1:]], 1).reshape(-1)
    for k, v in over.items():
        c[k] = np.asarray(v) if isinstance(c[k], np.ndarray) else v
    return c


def _run(exe, cases, tmp_path):
    """Per case a list over the F * B blocks of (frame fields or None, point fields or None)."""
    path = os.path.join(str(tmp_path), 'frame_cases.txt')
    with open(path, 'w') as fh:
        for c in cases:
            fh.write('%d %d %d %d %d %d\n' % tuple(c[k] for k in ('F', 'B', 'n_lig', 'n_half', 'n_point', 'n_out')))
            for k in ('lig_off', 'bond_off', 'range', 'out_off'):
                fh.write(' '.join(str(int(v)) for v in c[k]) + '\n')
    lines = iter(run_program(exe, 'frames', path)[:-1])               # (without the empty piece after the last newline)
    got = []
    for c in cases:
        rows = []
        for _ in range(c['F'] * c['B']):
            v = [int(x) for x in next(lines).split()]
            frame = dict(zip(('f', 'g', 'a0', 'n', 'h0', 'n_pair', 'arow', 'hrow'), v[1:9])) if v[0] else None
            pts = dict(zip(('ps', 'pe', 'o0', 'orow'), v[10:14])) if v[0] and v[9] else None
            rows.append((frame, pts))
        got.append(rows)
    assert next(lines, None) is None
    return got


def _accepted(rows, B):
    """(graphs whose frame is accepted, graphs whose points are too): the same in every frame."""
    per_frame = [([g for g in range(B) if rows[f * B + g][0]], [g for g in range(B) if rows[f * B + g][1]]) for f in range(len(rows) // B)]
    assert all(p == per_frame[0] for p in per_frame)
    return per_frame[0]


SIZES, POINTS = (5, 128, 1), (4, 0, 7)


def test_guards_accept_a_well_formed_batch(exe, tmp_path):
    c = _case(SIZES, POINTS, F=3)
    (rows,) = _run(exe, [c], tmp_path)
    for f in range(3):
        for g, n in enumerate(SIZES):
            frame, pts = rows[f * 3 + g]
            a0, h0, o0 = sum(SIZES[:g]), sum(_pairs(m) for m in SIZES[:g]), sum(POINTS[:g])
            assert frame == dict(f=f, g=g, a0=a0, n=n, h0=h0, n_pair=_pairs(n), arow=f * c['n_lig'] + a0, hrow=f * c['n_half'] + h0)
            assert pts == dict(ps=o0, pe=o0 + POINTS[g], o0=o0, orow=f * c['n_out'] + o0)
    # all graphs share all points (point_batch=None): ranges [0, P) each, outputs B * P
    shared = _case(SIZES, (6, 6, 6), range=[0, 6] * 3, n_point=6)
    (rows,) = _run(exe, [shared], tmp_path)
    assert _accepted(rows, 3) == ([0, 1, 2], [0, 1, 2]) and rows[3 + 2][1] == dict(ps=0, pe=6, o0=12, orow=18 + 12)
    # empty graphs, no points at all
    (rows,) = _run(exe, [_case((0, 0, 0), (0, 0, 0))], tmp_path)
    assert _accepted(rows, 3) == ([0, 1, 2], [0, 1, 2])


def test_frame_guard_refuses_what_leaves_the_frame(exe, tmp_path):
    lig, bond = _case(SIZES, POINTS)['lig_off'], _case(SIZES, POINTS)['bond_off']
    cases = {
        'negative atom offset': (_case(SIZES, POINTS, lig_off=[-1, 5, 133, 134]), [1, 2]),
        'negative bond offset': (_case(SIZES, POINTS, bond_off=[-2, 20, 20 + 2 * _pairs(128), 20 + 2 * _pairs(128)]), [1, 2]),
        'atoms past the frame': (_case(SIZES, POINTS, n_lig=133), [0, 1]),                         # the last graph's one atom
        'pairs past the frame': (_case(SIZES, POINTS, n_half=10 + _pairs(128) - 1), [0]),          # (the last one starts past it)
        'a graph of 129 atoms': (_case((5, 129, 1), POINTS), [0, 2]),
        'decreasing offsets': (_case(SIZES, POINTS, lig_off=[0, 5, 3, 134]), [0]),                 # n = -2, then n = 131
        'all offsets beyond': (_case(SIZES, POINTS, lig_off=lig + 1000, bond_off=bond + 2000), []),
    }
    got = _run(exe, [c for c, _ in cases.values()], tmp_path)
    for (what, (c, want)), rows in zip(cases.items(), got):
        assert _accepted(rows, 3)[0] == want, what


def test_point_guard_refuses_what_leaves_the_points(exe, tmp_path):
    cases = {
        'end before start': (_case(SIZES, POINTS, range=[4, 0, 4, 4, 4, 11]), [1, 2]),
        'negative start': (_case(SIZES, POINTS, range=[-1, 3, 4, 4, 4, 11]), [1, 2]),
        'end past the points': (_case(SIZES, POINTS, n_point=10), [0, 1]),
        'output span of another length': (_case(SIZES, POINTS, out_off=[0, 5, 5, 12], n_out=12), [1, 2]),
        'output span shorter': (_case(SIZES, POINTS, range=[0, 4, 4, 4, 4, 11], out_off=[0, 4, 4, 10]), [0, 1]),
        'outputs past the frame': (_case(SIZES, POINTS, n_out=10), [0, 1]),
        'negative output offset': (_case(SIZES, POINTS, out_off=[-4, 0, 0, 7]), [1, 2]),
    }
    got = _run(exe, [c for c, _ in cases.values()], tmp_path)
    for (what, (c, want)), rows in zip(cases.items(), got):
        assert _accepted(rows, 3) == ([0, 1, 2], want), what
