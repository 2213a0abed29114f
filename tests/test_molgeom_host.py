"""CPU: the geometry screen's definition (restated in tests/geom_reference.py from DESIGN.md 2.9 "Geometry") on hand-built molecules
with hand-computed answers, the conditions of the generated batch, the limits' sources, the SDF data item, the binding.

The kernel itself is held against the restatement in tests/test_gpu_molgeom.py."""
import math
import os
import re

import numpy as np
import pytest
import torch

import geom_reference as G
from mol_support import arg_count, header_macro, header_text
from phoregen_amd import hip
from phoregen_amd import molecule as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float('inf')


def _order(n, bonds):
    o = np.zeros(n * (n - 1) // 2, dtype=np.int8)
    for (a, b), t in bonds.items():
        o[G.R.pair_row(a, b, n)] = t
    return o


def test_triangle_3_4_5_by_hand():
    pos = [[0, 0, 0], [3, 0, 0], [0, 4, 0]]
    r = G.geom_graph(pos, [1, 1, 3], _order(3, {(0, 1): 1, (0, 2): 2}), [[0, 0, 1], [3, 0, 3.5]], [0, 1])
    bond_max = float(np.float32(2.8))                                  # the limit as the kernel receives it
    assert r['metrics'][:5].tolist() == [3.0, 4.0, 5.0, 3.5, 1.0]
    assert r['metrics'][5] == pytest.approx(math.sqrt(34.0) / 3.0, rel=1e-15)      # (1, 4/3, 0) - (0, 0, 1)
    assert r['metrics'][6] == pytest.approx(((3.0 - bond_max) + (4.0 - bond_max)) / 2.0, rel=1e-15) and r['metrics'][7] == 0.0
    assert r['counts'].tolist() == [0, 2, 0, 0, 1, 1] and r['status'] == M.GEOM_BOND_LONG and not r['ok']
    assert r['point_dist'].tolist() == [1.0, 3.5] and r['point_atom'].tolist() == [0, 1]
    # a dropped atom in front: the compact index counts kept classes only, the dropped atom's coordinates play no part
    r2 = G.geom_graph([[0.1, 0.1, 1.0]] + pos, [11, 1, 1, 3], _order(4, {(1, 2): 1, (1, 3): 2, (0, 1): 1}), [[0, 0, 1], [3, 0, 3.5]], [0, 1])
    assert r2['metrics'].tolist() == r['metrics'].tolist() and r2['counts'].tolist() == r['counts'].tolist()
    assert r2['point_atom'].tolist() == [0, 1] and r2['status'] == r['status']


def test_comparisons_are_strict():
    """Distances exactly at a limit: 3 (bond_min), 4 (bond_max), 5 (clash_min), 5 to an exclusion sphere (ex_clear): no bit.  A
    feature exactly at feat_cut is NOT covered (`check_nearby_phore` compares with <), one just inside is."""
    pos, order = [[0, 0, 0], [3, 0, 0], [0, 4, 0]], _order(3, {(0, 1): 1, (0, 2): 1})
    lim = (3.0, 4.0, 5.0, 5.0, 2.0)
    r = G.geom_graph(pos, [1, 1, 1], order, [[0, 0, 1], [0, 0, -5]], [0, 1], lim)
    assert r['status'] == 0 and r['counts'].tolist() == [0, 0, 0, 0, 1, 1] and r['metrics'][6] == 0.0
    r = G.geom_graph(pos, [1, 1, 1], order, [[0, 0, 2], [0, 0, -5]], [0, 1], lim)
    assert r['status'] == M.GEOM_FEATURE_MISSED and r['counts'].tolist() == [0, 0, 0, 0, 0, 1] and r['ok']
    # one representable step inside each limit sets its bit
    eps = 2.0 ** -20
    tight = (3.0 + eps, 4.0 - eps, 5.0 + eps, 5.0 + eps, 2.0 + eps)
    r = G.geom_graph(pos, [1, 1, 1], order, [[0, 0, 2], [0, 0, -5]], [0, 1], tight)
    assert r['status'] == M.GEOM_BOND_SHORT | M.GEOM_BOND_LONG | M.GEOM_CLASH | M.GEOM_EX_CLASH and r['counts'].tolist() == [1, 1, 1, 1, 1, 1]


def test_each_status_bit_alone():
    bond = _order(2, {(0, 1): 1})
    feat, ex = [0.5, 0, 0], [0, 6, 0]

    def two(d, order=bond, points=(feat, ex)):
        return G.geom_graph([[0, 0, 0], [d, 0, 0]], [1, 3], order, list(points), [0, 1])
    assert two(1.5)['status'] == 0 and two(1.5)['ok']
    assert two(1.0)['status'] == M.GEOM_BOND_SHORT and two(1.0)['metrics'][6] == pytest.approx(float(np.float32(1.2)) - 1.0)
    assert two(2.9)['status'] == M.GEOM_BOND_LONG
    assert two(1.0, order=_order(2, {}))['status'] == M.GEOM_CLASH and two(1.5, order=_order(2, {}))['status'] == 0
    r = two(1.5, points=(feat, [-2.5, 0, 0]))
    assert r['status'] == M.GEOM_EX_CLASH and r['counts'][3] == 1 and r['metrics'][3] == 2.5     # atom 1 is 4.0 away
    r = two(1.5, points=([0, 0, 2.5], ex))
    assert r['status'] == M.GEOM_FEATURE_MISSED and r['ok'] and r['metrics'][4] == 2.5
    r = G.geom_graph([[0, 0, 0], [1.5, 0, 0], [np.nan, 0, 0]], [1, 3, 1], _order(3, {(0, 1): 1, (1, 2): 1}), [feat, ex], [0, 1])
    assert r['status'] == M.GEOM_NONFINITE and not r['ok'] and r['n_kept'] == 2 and r['n_bond'] == 1
    r = G.geom_graph([[0, 0, 0], [1.5, 0, 0]], [1, 3], bond, [feat, ex, [0, np.inf, 0]], [0, 1, 0])
    assert r['status'] == M.GEOM_NONFINITE and r['counts'].tolist() == [0, 0, 0, 0, 1, 1]
    assert r['point_dist'].tolist() == [0.5, 6.0, INF] and r['point_atom'].tolist() == [0, 0, -1]
    # nothing kept / nothing to measure against
    r = G.geom_graph([[0, 0, 0]], [11], _order(1, {}), [feat, ex], [0, 1])
    assert r['metrics'][:5].tolist() == [INF, -INF, INF, INF, INF] and math.isnan(r['metrics'][5]) and r['metrics'][6] == 0.0
    assert r['status'] == M.GEOM_FEATURE_MISSED and r['point_atom'].tolist() == [-1, -1]
    r = G.geom_graph([[0, 0, 0]], [1], _order(1, {}), np.zeros((0, 3)), [])
    assert r['metrics'][:5].tolist() == [INF, -INF, INF, INF, -INF] and math.isnan(r['metrics'][5]) and r['status'] == 0
    assert M.GEOM_FAIL_MASK == 1 | 2 | 4 | 8 | 32 and sorted(M.GEOM_NAMES) == [1, 2, 4, 8, 16, 32]


def test_generated_batch_meets_its_conditions():
    """Judged by the restatement alone; tests/test_gpu_molgeom.py asserts the same before it looks at the kernel."""
    batch = G.generate_batch()
    census = G.check_batch(batch, G.restate_batch(batch))
    print('census of the generated batch:', census)


def test_limits_are_the_reference_values():
    lim = M.GeomLimits()
    assert (lim.bond_min, lim.bond_max) == (1.2, 2.8)                  # compute_atom_prox_loss(min_d=1.2, max_d=2.8)
    assert lim.feat_cut == 2.0                                         # check_nearby_phore(cutoff=2)
    assert lim.ex_clear == 3.0                                         # exclude_clashed_ex(low=3.0)
    assert lim.clash_min == lim.bond_min                               # no reference value: the one-sided rule of DESIGN.md 2.9
    assert G.limits64().tolist() == [float(np.float32(v)) for v in (1.2, 2.8, 1.2, 3.0, 2.0)]
    assert len(M.GEOM_METRICS) == 8 and len(M.GEOM_COUNTS) == 6


def test_write_sdf_geom_item(tmp_path):
    from test_molecule_host import ETHANOL, ETHANOL_BLOCK
    geom = dict(zip(M.GEOM_METRICS, [1.43, 1.5123456, 2.4, INF, -INF, float('nan'), 0.00004, 0.0]), status=M.GEOM_FEATURE_MISSED | M.GEOM_CLASH,
                geom_ok=False)
    path = tmp_path / 'g.sdf'
    M.write_sdf(str(path), [dict(ETHANOL, geom=geom, key=0x1F), ETHANOL], names=['ethanol'] * 2)
    item = ('> <PHOREGEN_GEOM>\nstatus 0x14\nbond_min 1.4300\nbond_max 1.5123\nnonbonded_min 2.4000\nex_min inf\nfeature_max -inf\n'
            'centre_dist nan\nbond_energy 0.0000\n\n')
    assert path.read_text() == ETHANOL_BLOCK + '> <PHOREGEN_KEY>\n000000000000001f\n\n' + item + '$$$$\n' + ETHANOL_BLOCK + '$$$$\n'


def test_geometry_needs_the_device():
    node, pos, edge, _ = G.R.scores_from_classes([1, 3], {(0, 1): 1})
    res = {'pred': [node, pos, edge], 'traj': [None, None, None], 'lig_info': [torch.tensor([2])]}
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        M.geometry(res, torch.zeros(1, 3), torch.zeros(1))
    data = type('D', (dict,), {})({'phore': type('P', (), {'pos': torch.zeros(2, 3), 'x': torch.zeros(2, 13)})()})
    data.center = torch.ones(3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        M.geometry_for(data, res)


def test_binding_declares_the_geometry_screen():
    lib = hip.load_library()
    header = header_text()
    assert re.search(r'\bint pg_mol_geom\s*\(', header)
    assert 'pg_mol_geom' in hip.EXPORTS and hasattr(lib, 'pg_mol_geom')
    assert len(hip._PROTOS['pg_mol_geom'][1]) == 24 == arg_count('pg_mol_geom')
    assert hip.ABI_VERSION == 11 == lib.pg_abi_version()
    assert 'mol_geom.hip' in open(os.path.join(ROOT, 'phoregen_amd', 'csrc', 'Makefile')).read()
    for bit, name in M.GEOM_NAMES.items():
        assert header_macro('PG_GEOM_' + name) == str(bit), name
    # argument errors are refused before any launch, without a GPU: oversize, negative sizes, no limits
    lim = (hip.C.c_float * 5)(1.2, 2.8, 1.2, 3.0, 2.0)
    args = lambda B, n_lig, n_bond, max_n, n_point=0, limits=lim: (None, 0, None, None, None, None, B, 1, n_lig, n_bond, max_n, None, None,   # noqa: E731
                                                                  n_point, None, None, 0, limits, None, None, None, None, None, None)
    assert lib.pg_mol_geom(*args(1, M.MAX_ATOMS + 1, 0, M.MAX_ATOMS + 1)) != 0 and b'PG_MOL_MAX_ATOMS' in lib.pg_last_error()
    assert lib.pg_mol_geom(*args(1, 4, 12, -1)) != 0 and b'pg_mol_geom' in lib.pg_last_error()
    assert lib.pg_mol_geom(*args(1, 4, 12, 4, n_point=-1)) != 0
    assert lib.pg_mol_geom(*args(1, 4, 12, 4, limits=None)) != 0 and b'limits' in lib.pg_last_error()
    assert lib.pg_mol_geom(*args(0, 0, 0, 0)) == 0
