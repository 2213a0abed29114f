"""-m gpu: the property kernel (csrc/mol_props.hip through phoregen_amd/properties.py) against the plain restatement of
tests/props_reference.py, which is fed the device's own Kekulé and ring arrays (screen -> kekulize -> rings -> properties).  Integer
work only: every comparison is `==` on every output array."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import props_reference as PR
from mol_support import C_, N_, O_, batch_from, chain, cycle, mol_result as _result, permute_batch, split_frame
from phoregen_amd import hip
from phoregen_amd import molecule as M
from phoregen_amd import properties as P
from phoregen_amd import scaffold as SC
from test_molprops_host import HAND

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ('status', 'counts', 'ok', 'atom_env', 'atom_row', 'sums', 'weight_milli', 'violated')
HAND_TABLE = P.PropertyTable('hand', HAND)
CYCLOPENTADIENYL = ([C_] * 5, cycle(5, 4))                              # five aromatic carbons: no Kekulé structure


def _split(pr, sizes, f=0):
    """Frame f of a `Properties` (with the inputs the kernel read) as one dict of numpy values per graph."""
    out = split_frame(sizes, f, per_atom={'atom_env': pr.atom_env, 'cls': pr.screen.cls, 'hcount': pr.kekule.hcount, 'charge': pr.kekule.charge,
                                          'atom_ring': pr.rings.atom_ring},
                      per_pair={'order': pr.screen.order, 'kekule_order': pr.kekule.kekule_order, 'ring_size': pr.rings.ring_size},
                      per_graph={'status': pr.status, 'counts': pr.counts, 'ok': pr.ok, 'sums': pr.sums, 'weight_milli': pr.weight_milli,
                                 'violated': pr.violated, 'kekule_status': pr.kekule.status})
    rows, n0 = pr.atom_row[f].cpu().numpy(), 0
    for r, n in zip(out, sizes):
        r['atom_row'] = rows[:, n0:n0 + n]
        n0 += n
    return out


def _restate(r, pr):
    return PR.properties_of_rows(r['cls'], r['order'], r['kekule_order'], r['hcount'], r['charge'], r['kekule_status'], r['ring_size'],
                                 r['atom_ring'], [list(t.rows) for t in pr.tables], pr.limits.pairs(pr.tables), pr.limits.max_violations)


def _same(got, want, where=''):
    for k in ('status', 'weight_milli', 'violated', 'ok'):
        assert got[k] == want[k], (where, k, got[k], want[k])
    assert got['counts'].tolist() == want['counts'].tolist(), (where, dict(zip(PR.COUNTS, zip(got['counts'].tolist(), want['counts'].tolist()))))
    assert got['sums'].tolist() == want['sums'].tolist(), (where, got['sums'], want['sums'])
    for k in ('atom_env', 'atom_row'):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (where, k, np.nonzero(got[k] != want[k]))


def _run(graphs, tables=P.DEFAULT_TABLES, limits=P.PropertyLimits(), where=''):
    """The kernel on one frame == the restatement on the device's Kekulé form and rings; returns (result, Properties, per-graph rows)."""
    node, pos, edge, sizes = batch_from(graphs)
    res = _result(node, pos, edge, sizes)
    pr = P.properties(res, tables=tables, limits=limits)
    torch.cuda.synchronize()
    N, B = sum(sizes), len(sizes)
    assert pr.tables == tuple(tables) and pr.limits == limits and pr.kekule.screen is pr.screen and pr.rings.screen is pr.screen
    assert [(tuple(getattr(pr, k).shape), getattr(pr, k).dtype) for k in OUTPUTS] == [
        ((1, B), torch.int32), ((1, B, 16), torch.int32), ((1, B), torch.bool), ((1, N), torch.int32), ((1, 4, N), torch.uint8),
        ((1, B, 4), torch.int32), ((1, B), torch.int32), ((1, B), torch.int32)]
    rows = _split(pr, sizes)
    for g, r in enumerate(rows):
        _same(r, _restate(r, pr), '%s graph %d of %d atoms' % (where, g, sizes[g]))
    return res, pr, rows


def _hetero_chain(n):
    classes = [C_] * n
    for i in range(3, n, 8):
        classes[i] = N_
    for i in range(7, n, 8):
        classes[i] = O_
    return classes, chain(n, 1)


def test_mask_word_and_lane_boundaries():
    tail = ([O_] + [C_] * 126, {**cycle(3, 1), **{(i, i + 1): 1 for i in range(2, 126)}})                # a 3-ring with a tail of 124
    benzyl = lambda n: ([C_] * n, {**cycle(6, 4), **{(i, i + 1): 1 for i in range(5, n - 1)}})         # noqa: E731  (benzene with a chain)
    graphs = [([], {}), ([C_], {}), ([C_, O_], {(0, 1): 1}), ([O_, C_, C_], cycle(3, 1)), _hetero_chain(63), benzyl(64), _hetero_chain(65), tail,
              ([C_] * 128, chain(128, 1)), benzyl(128)]
    _, pr, rows = _run(graphs, limits=P.PropertyLimits.veber(), where='boundaries')
    assert [len(r['atom_env']) for r in rows] == [0, 1, 2, 3, 63, 64, 65, 127, 128, 128]
    c = lambda g, k: int(rows[g]['counts'][PR.COUNTS.index(k)])       # noqa: E731
    assert rows[0]['status'] == 0 and rows[0]['counts'].tolist() == [0] * 16 and rows[0]['weight_milli'] == 0
    assert c(1, 'hydrogens') == 4 and rows[1]['weight_milli'] == 16043 and c(8, 'rotatable') == 125 and c(8, 'hydrogens') == 258
    assert c(7, 'ring_atoms') == 3 and PR.unpack(int(rows[7]['atom_env'][0]))['ring3'] == 1 and c(7, 'rotatable') == 123
    assert rows[8]['violated'] == 1 << 4 and not rows[8]['ok'] and rows[3]['ok'] and not rows[5]['ok'] and c(9, 'aromatic_atoms') == 6
    assert all(c(g, 'untyped') == 0 and not rows[g]['status'] & P.PROP_NO_KEKULE for g in range(10))
    # the outputs do not depend on what their buffers held: a call into recycled memory agrees
    again = P.properties(_result(*batch_from(graphs)[:3], [len(g[0]) for g in graphs]), limits=P.PropertyLimits.veber())
    assert all(torch.equal(getattr(pr, k), getattr(again, k)) for k in OUTPUTS)


def test_named_molecules_and_the_random_family_under_both_presets():
    names = list(PR.NAMED)
    graphs = PR.named_graphs() + PR.random_family()
    for limits in (P.PropertyLimits.lipinski(), P.PropertyLimits.veber()):
        _, pr, rows = _run(graphs, limits=limits, where='family')
        assert not any(r['status'] & P.PROP_UNTYPED for r in rows)
    assert sum(not r['status'] & P.PROP_NO_KEKULE for r in rows) * 2 >= len(rows)
    # the hand-written answers, on the device's own Kekulé form
    _, pr, rows = _run(graphs[:len(names)], tables=(HAND_TABLE,), where='named')
    for k, r in zip(names, rows):
        _, _, fields, hand_rows, counts, weight = PR.NAMED[k]
        assert r['atom_env'].tolist() == [PR.pack(f) for f in fields], k
        assert r['atom_row'][0].tolist() == [255 if x is None else x for x in hand_rows] and r['weight_milli'] == weight, k
        assert dict(zip(PR.COUNTS, r['counts'].tolist())) == dict(dict.fromkeys(PR.COUNTS, 0), **counts, untyped=sum(x is None for x in hand_rows)), k
    assert pr.mol_weight[0, 0].item() == 46.069 and pr.value('hand')[0, 0].item() == 1.875 and pr.fsp3[0, :6].tolist() == [1.0, 0.5, 0.5, 2 / 3, 2 / 3, 0.0]


def test_alone_and_in_a_renumbered_batch():
    graphs = PR.random_family()[::3] + [PR.NAMED[k][:2] for k in ('N-methylacetamide', 'pyridine', 'tetramethylammonium')] + [CYCLOPENTADIENYL]
    node, pos, edge, sizes = batch_from(graphs)
    _, pr, rows = _run(graphs, limits=P.PropertyLimits.lipinski(), where='batch')
    for g in (0, 3, len(graphs) - 2):                                   # a graph's rows do not depend on its batch
        _, _, alone = _run([graphs[g]], limits=P.PropertyLimits.lipinski(), where='alone')
        _same(alone[0], {k: rows[g][k] for k in OUTPUTS}, 'alone %d' % g)
    node2, pos2, edge2, perms = permute_batch(node, pos, edge, sizes, seed=5)
    pr2 = P.properties(_result(node2, pos2, edge2, sizes), limits=P.PropertyLimits.lipinski())
    rows2, checked = _split(pr2, sizes), 0
    for g, (a, b, p) in enumerate(zip(rows, rows2, perms)):
        _same(b, _restate(b, pr2), 'renumbered %d' % g)
        if (a['kekule_status'] | b['kekule_status']) & M.KEKULE_CHARGED:
            continue                                                   # (which atom carries the charge depends on the matching)
        checked += 1
        for k in ('status', 'weight_milli', 'violated', 'ok'):
            assert a[k] == b[k], (g, k)
        assert a['counts'].tolist() == b['counts'].tolist() and a['sums'].tolist() == b['sums'].tolist(), g
        assert sorted(a['atom_env'].tolist()) == sorted(b['atom_env'].tolist()), g
        assert b['atom_env'][p].tolist() == a['atom_env'].tolist() and b['atom_row'][:, p].tolist() == a['atom_row'].tolist(), g
    assert checked >= len(graphs) - 3


def test_trajectory_frames_in_one_launch():
    names = [['ethanol', 'benzene', 'acetamide'], ['oxirane', 'pyridine', 'acetic acid'], ['butane', 'phenol', 'acetonitrile']]
    pad = (4, 7, 5)
    frames = [[(list(PR.NAMED[k][0]) + [O_] * (n - len(PR.NAMED[k][0])), PR.NAMED[k][1]) for k, n in zip(row, pad)] for row in names]
    per = [batch_from(f) for f in frames]
    sizes = per[0][3]
    traj = []
    for k in range(3):                                                 # frames that are not dense in memory
        rows, width = per[0][k].shape
        big = torch.full((3, rows + 4, width), 0.5, device=DEV)
        big[:, :rows] = torch.stack([p[k] for p in per]).to(DEV)
        traj.append(big[:, :rows])
    res = _result(*per[-1][:3], sizes, traj=tuple(traj))
    lim = P.PropertyLimits(heavy_atoms=(None, 5))
    pr = P.properties(res, frames='traj', limits=lim)
    assert pr.atom_env.shape == (3, 16) and pr.atom_row.shape == (3, 4, 16) and pr.counts.shape == (3, 3, 16)
    for f, p in enumerate(per):
        alone = P.properties(_result(*p[:3], sizes), limits=lim)
        assert all(torch.equal(getattr(pr, k)[f], getattr(alone, k)[0]) for k in OUTPUTS), f
        for g, r in enumerate(_split(pr, sizes, f)):
            _same(r, _restate(r, pr), 'frame %d graph %d' % (f, g))
    assert pr.counts[:, :, 0].tolist() == [[4, 7, 5]] * 3 and pr.ok.tolist() == [[True, False, True]] * 3


def test_zero_one_and_four_tables_and_the_row_limits():
    graphs = [PR.NAMED[k][:2] for k in ('N-methylacetamide', 'phenol', 'dimethyl sulfone')] + PR.random_family()[:4]
    empty = P.PropertyTable('empty')
    last = P.PropertyTable('last', [(1 << 30, 1 << 30, 1, 1)] * 127 + [(0, 0, 70, 3)])       # 128 rows, the last one the only match
    _, pr0, rows0 = _run(graphs, tables=(), where='no table')
    assert (pr0.sums == 0).all() and (pr0.atom_row == 255).all() and (pr0.counts[..., hip.PG_PROP_C_UNTYPED] == 0).all()
    _run(graphs, tables=(P.LOGP,), limits=P.PropertyLimits(sums={'logp': (0.0, 3.0)}), where='one table')
    _, pr4, rows4 = _run(graphs, tables=(HAND_TABLE, empty, last, P.TPSA_SP), limits=P.PropertyLimits(sums={'last': (None, 0.05)}), where='four tables')
    kept = pr4.atom_env[0] >= 0
    assert (pr4.atom_row[0, 1] == 255).all() and (pr4.atom_row[0, 2][kept] == 127).all() and (pr4.sums[0, :, 1] == 0).all()
    r = rows4[0]
    assert r['sums'][2] == 5 * 70 + 7 * 3 and r['counts'][hip.PG_PROP_C_UNTYPED] == 1 + 5 and r['violated'] == 0 and rows4[1]['violated'] == 1 << 7
    assert [x['atom_env'].tolist() for x in rows0] == [x['atom_env'].tolist() for x in rows4]
    # 5 tables and 129 rows: the Python classes refuse them, and so does the library when they are handed to it directly
    with pytest.raises(ValueError, match='at most MAX_TABLES = 4'):
        P.properties(_result(*batch_from(graphs)[:3], [len(g[0]) for g in graphs]), tables=(P.TPSA, P.LOGP, P.MR, empty, last))
    with pytest.raises(ValueError, match='MAX_ROWS = 128'):
        P.PropertyTable('long', [(0, 0, 0, 0)] * 129)
    out = {k: torch.full_like(getattr(pr4, k), 77) for k in OUTPUTS if k != 'ok'}
    weights = torch.tensor(P.weight_table(), dtype=torch.int32, device=DEV)
    B, sc = len(graphs), pr4.screen
    launch = lambda rows: P._launch_props(hip.lib(), sc, pr4.kekule, pr4.rings, B, 1, max(sc.num_atoms),          # noqa: E731
                                          torch.zeros(sum(rows), 4, dtype=torch.int32, device=DEV), rows, weights, PR.NO_LIMITS, 0, out)
    with pytest.raises(RuntimeError, match='table 1 has 129 rows'):
        launch([3, 129])
    with pytest.raises(RuntimeError, match='5 tables'):
        launch([1] * 5)
    torch.cuda.synchronize()
    assert all((t == 77).all() for t in out.values())


def test_oversize_graph_cpu_result_and_empty_batch():
    n = M.MAX_ATOMS + 1
    h = n * (n - 1) // 2
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)      # noqa: E731
    sc = M.Screen(status=z((1, 1), torch.int32), counts=z((1, 1, 4), torch.int32), valid=z((1, 1), torch.bool), cls=z((1, n), torch.int8),
                  compact=z((1, n), torch.int16), valence2=z((1, n), torch.uint8), comp=z((1, n), torch.int16), order=z((1, h), torch.int8),
                  lig_off=torch.tensor([0, n], dtype=torch.int32, device=DEV), bond_off=torch.tensor([0, 2 * h], dtype=torch.int32, device=DEV),
                  num_atoms=[n])
    kek = M.Kekule(status=z((1, 1), torch.int32), counts=z((1, 1, 10), torch.int32), ok=z((1, 1), torch.bool), kekule_order=z((1, h), torch.int8),
                   hcount=z((1, n), torch.uint8), charge=z((1, n), torch.int8), options=M.KekuleOptions(), screen=sc)
    rg = M.Rings(status=z((1, 1), torch.int32), counts=z((1, 1, len(M.RING_COUNTS)), torch.int32), ok=z((1, 1), torch.bool),
                 ring_size=z((1, h), torch.uint8), atom_ring=z((1, n), torch.uint8), ring_sys=z((1, n), torch.int16), limits=M.RingLimits(), screen=sc)
    full = lambda shape, dt: torch.full(shape, 77, dtype=dt, device=DEV)   # noqa: E731
    out = dict(status=full((1, 1), torch.int32), counts=full((1, 1, 16), torch.int32), atom_env=full((1, n), torch.int32),
               atom_row=full((1, 4, n), torch.uint8), sums=full((1, 1, 4), torch.int32), weight_milli=full((1, 1), torch.int32),
               violated=full((1, 1), torch.int32))
    packed = torch.from_numpy(P.pack_tables(P.DEFAULT_TABLES)).to(DEV)
    weights = torch.tensor(P.weight_table(), dtype=torch.int32, device=DEV)
    rows = [len(t.rows) for t in P.DEFAULT_TABLES]
    with pytest.raises(RuntimeError) as err:
        P._launch_props(hip.lib(), sc, kek, rg, 1, 1, n, packed, rows, weights, PR.NO_LIMITS, 0, out)
    assert 'PG_MOL_MAX_ATOMS' in str(err.value) and 'pg_mol_props' in str(err.value) and str(n) in str(err.value)
    with pytest.raises(ValueError, match='do not fit'):
        P._launch_props(hip.lib(), sc, kek, rg, 1, 1, 8, packed, rows, weights, PR.NO_LIMITS, 0, dict(out, atom_env=out['atom_env'][:, :5].contiguous()))
    torch.cuda.synchronize()
    assert all((t == 77).all() for t in out.values())
    node, pos, edge, sizes = batch_from([PR.NAMED['ethanol'][:2]])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        P.properties(_result(node, pos, edge, sizes, dev='cpu'))
    res = _result(node, pos, edge, sizes)
    other = M.screen(_result(*batch_from([PR.NAMED['benzene'][:2]])[:3], [6]))
    with pytest.raises(ValueError, match='screens of different results'):
        P.properties(res, kekule=M.kekulize(res), rings=M.rings(_result(*batch_from([PR.NAMED['benzene'][:2]])[:3], [6]), screen=other))
    with pytest.raises(ValueError, match="names the table 'logp'"):
        P.properties(res, tables=(P.TPSA,), limits=P.PropertyLimits.lipinski())
    with pytest.raises(ValueError, match='limits must be a PropertyLimits'):
        P.properties(res, limits='lipinski')
    empty = P.properties(_result(torch.zeros(0, 12), torch.zeros(0, 3), torch.zeros(0, 6), []))
    assert empty.atom_env.shape == (1, 0) and empty.counts.shape == (1, 0, 16) and empty.atom_row.shape == (1, 4, 0)


def test_a_graph_without_a_kekule_structure_fails_alone():
    graphs = [PR.NAMED['phenol'][:2], CYCLOPENTADIENYL, PR.NAMED['acetic acid'][:2]]
    _, pr, rows = _run(graphs, limits=P.PropertyLimits(heavy_atoms=(6, None)), where='failed')
    assert int(pr.kekule.status[0, 1]) & M.KEKULE_FAILED and pr.status[0].tolist() == [0, P.PROP_NO_KEKULE, P.PROP_LIMITS]
    r = rows[1]
    assert r['atom_env'].tolist() == [-1] * 5 and (r['atom_row'] == 255).all() and r['counts'].tolist() == [0] * 16
    assert r['sums'].tolist() == [0] * 4 and r['weight_milli'] == 0 and r['violated'] == 0 and not r['ok']
    assert pr.ok[0].tolist() == [True, False, False] and rows[2]['violated'] == 2
    _, _, alone = _run([graphs[0]], limits=P.PropertyLimits(heavy_atoms=(6, None)))
    _same(alone[0], {k: rows[0][k] for k in OUTPUTS}, 'the neighbour')


def test_assemble_and_write_sdf_carry_the_properties(tmp_path):
    graphs = [PR.NAMED[k][:2] for k in ('N-methylacetamide', 'chlorobenzene')] + [(PR.NAMED['benzene'][0] + [11], PR.NAMED['benzene'][1])]
    res, pr, rows = _run(graphs, limits=P.PropertyLimits.lipinski())
    plain, full = M.assemble(res), M.assemble(res, properties=pr, kekule=pr.kekule)
    for m, p, r in zip(full, plain, rows):
        assert list(m) == list(p) + ['kekule', 'properties']
        q, keep = m['properties'], r['cls'] >= 0
        assert q['status'] == r['status'] and q['properties_ok'] == bool(r['ok']) and [q[k] for k in PR.COUNTS[:-1]] == r['counts'][:-1].tolist()
        assert q['mol_weight'] == r['weight_milli'] / 1000 and [q['tpsa'], q['logp'], q['mr']] == [s / 1e4 for s in r['sums'][:3].tolist()]
        assert q['env'].tolist() == r['atom_env'][keep].tolist() and q['row'].tolist() == r['atom_row'][:3].T[keep].tolist()
        assert abs(q['mol_weight'] - m['kekule']['mol_weight']) < 1e-6   # (the host's sum of the same table)
    assert [len(m['properties']['env']) for m in full] == [5, 7, 6] and full[0]['properties']['amide_bonds'] == 1
    # the command-line tool's file of the same molecules (its own run below finishes none under the synthetic weights)
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import sample_cli
    sample_cli.write_property_file(str(tmp_path), 'x', full)
    lines = (tmp_path / 'x_properties.txt').read_text().split('\n')
    assert lines[0] == '# index mol_weight tpsa logp mr nhoh no_count rotatable heavy_atoms fsp3 status' and lines[-1] == '' and len(lines) == 5
    assert lines[1] == '0 73.095 29.1000 %.4f %.4f 1 2 0 5 0.6667 0x00' % (full[0]['properties']['logp'], full[0]['properties']['mr'])
    for i, (ln, m) in enumerate(zip(lines[1:], full)):
        q, w = m['properties'], ln.split()
        assert len(w) == 11 and int(w[0]) == i and float(w[1]) == q['mol_weight'] and int(w[10], 16) == q['status'] and float(w[9]) == round(q['fsp3'], 4)
        assert [int(x) for x in w[5:9]] == [q[k] for k in ('nhoh', 'no_count', 'rotatable', 'heavy_atoms')]
    with pytest.raises(ValueError, match='properties='):
        M.assemble(res, properties=P.properties(_result(*batch_from(graphs[:1])[:3], [5])))
    path = tmp_path / 'p.sdf'
    M.write_sdf(str(path), full)
    text = path.read_text()
    assert text.count('> <PHOREGEN_PROPERTIES>\nstatus 0x00\nmol_weight ') == 3 and 'mol_weight 73.095\ntpsa 29.1000\n' in text
    items = [rec.split('> <PHOREGEN_PROPERTIES>\n')[1].split('\n\n')[0] for rec in text.split('$$$$\n')[:-1]]
    for item, m in zip(items, full):                                   # the item reads back as the molecule's entries
        back = dict(ln.split(' ', 1) for ln in item.split('\n'))
        q = m['properties']
        assert int(back['status'], 16) == q['status'] and float(back['mol_weight']) == q['mol_weight'] and back['violated'] == '-'
        assert all(int(back[k]) == q[k] for k in PR.COUNTS[:-1]) and all(float(back[k]) == round(q[k], 4) for k in ('tpsa', 'logp', 'mr', 'fsp3'))


def test_sample_valid_tops_up_until_enough_molecules_pass():
    names = ['ethanol', 'chlorobenzene', 'butane', 'phenol', 'acetonitrile', 'benzene']
    parts = [batch_from([PR.NAMED[k][:2]]) for k in names]
    limits = P.PropertyLimits(heavy_atoms=(5, None))                   # the restatement: half of the stand-in's molecules pass
    passes = [PR.properties_of(*PR.NAMED[k][:2], [list(t.rows) for t in P.DEFAULT_TABLES], limits.pairs(P.DEFAULT_TABLES))['ok'] for k in names]
    assert passes == [False, True, False, True, False, True]

    class Rota:
        i = 0

        def sample(self, data, n, device, **kw):
            pick = [parts[(self.i + j) % len(parts)] for j in range(n)]
            self.i += n
            return _result(*(torch.cat([p[k] for p in pick]) for k in range(3)), [p[3][0] for p in pick])
    out = M.sample_valid(Rota(), None, num_samples=4, batch_size=3, properties=limits, max_failed_factor=3)
    assert len(out['finished']) == 4 and out['n_calls'] >= 3 and len(out['failed']) >= 3
    assert all(m['valid'] and m['properties']['properties_ok'] and m['properties']['heavy_atoms'] >= 5 for m in out['finished'])
    assert all(not m['properties']['properties_ok'] and m['properties']['violated_names'] == ('heavy_atoms',) for m in out['failed'])
    assert [m['properties']['heavy_atoms'] for m in out['finished']] == [7, 7, 6, 7] and 'kekule' not in out['finished'][0]
    lip = M.sample_valid(Rota(), None, num_samples=3, batch_size=3, properties=P.PropertyLimits.lipinski())
    assert len(lip['finished']) == 3 and not lip['failed'] and lip['n_calls'] == 1
    assert 'properties' not in M.sample_valid(Rota(), None, num_samples=1, batch_size=1)['finished'][0]


def test_finished_molecules_go_back_to_the_device():
    """`scaffold.batch_of` reaches this analysis too: the properties of assembled molecules are those of the draw."""
    graphs = [PR.NAMED[k][:2] for k in ('pyridine', 'methyl acetate', 'oxirane')]
    res, pr, _ = _run(graphs)
    back = P.properties(SC.batch_of(M.assemble(res), DEV))
    assert all(torch.equal(getattr(pr, k), getattr(back, k)) for k in OUTPUTS)


def test_sample_cli_writes_the_property_file_and_the_data_item(tmp_path):
    lst = tmp_path / 'files.json'
    lst.write_text(json.dumps([os.path.join(ROOT, 'tests', 'data', 'synthetic_test.phore')]))
    out = tmp_path / 'out'
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'sample_cli.py'), '--phore_file_list', str(lst), '--num_samples', '3',
                          '--batch_size', '3', '--outdir', str(out), '--properties', '--property_limits', '{"preset": "lipinski"}', '--sdf',
                          '--num_steps', '10'], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    done = torch.load(str(next(out.glob('*.pt'))), weights_only=False)
    (path,) = out.glob('*_properties.txt')
    lines = path.read_text().split('\n')[:-1]
    assert lines[0] == '# index mol_weight tpsa logp mr nhoh no_count rotatable heavy_atoms fsp3 status' and len(lines) == len(done) + 1
    for i, (ln, m) in enumerate(zip(lines[1:], done)):
        q, w = m['properties'], ln.split()
        assert q['properties_ok'] and len(w) == 11 and int(w[0]) == i and float(w[1]) == q['mol_weight'] and int(w[10], 16) == q['status']
        assert [float(x) for x in w[2:5]] == [round(q[k], 4) for k in ('tpsa', 'logp', 'mr')]
        assert [int(x) for x in w[5:9]] == [q[k] for k in ('nhoh', 'no_count', 'rotatable', 'heavy_atoms')]
    # the figures are those of the finished molecules, computed again here
    again = P.properties(SC.batch_of(done, DEV), limits=P.PropertyLimits.lipinski())
    assert again.weight_milli[0].tolist() == [round(m['properties']['mol_weight'] * 1000) for m in done]
    sdfs = sorted((out / 'sdf_results').glob('*.sdf'))
    assert len(sdfs) == len(done) and all('> <PHOREGEN_PROPERTIES>\nstatus 0x' in p.read_text() for p in sdfs)
