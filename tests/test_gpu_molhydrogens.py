"""-m gpu: the hydrogen kernel (csrc/mol_hydrogens.hip) through phoregen_amd/hydrogens.py against the float64 restatement of
tests/hydrogen_reference.py, and the functions that carry its answers.  The restatement is always fed the device's own screen and
Kekulé form, so only the kernel under test enters.  Integers compare with `==`; positions within the bound derived in
hydrogen_reference.py; the inputs keep every float-decided branch away from its threshold (asserted on the restatement alone in
tests/test_molhydrogens_host.py), which is why contacts are compared at clash_min 0.1, 0.4 and 16 and not at the default."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hydrogen_reference as H
from mol_support import MolRows, bits, read_mol_block, split_frame, mol_result as _result, permute_batch as _permute_batch
from phoregen_amd import hip, hydrogens as HY, molecule as M

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY_OPT = HY.HydrogenOptions(clash_min=H.FAMILY_CLASH)
NAMES = ('status', 'counts', 'h_pos', 'h_placed', 'site_shape', 'min_contact')


@pytest.fixture(scope='module')
def family():
    """The generated family: built once, read by several tests, changed by none."""
    return H.family()[0]


def _split(hy, pos, sizes, f=0):
    """Frame f of a `Hydrogens` as one dict of host values per graph, with 'rows' = the `all_rows` record of the device's own inputs."""
    sc, kk = hy.screen, hy.kekule
    out = split_frame(sizes, f, per_atom={'h_pos': hy.h_pos, 'h_placed': hy.h_placed, 'site_shape': hy.site_shape},
                      per_graph={'status': hy.status, 'counts': hy.counts, 'min_contact': hy.min_contact})
    rows = split_frame(sizes, f, per_atom={'cls': sc.cls, 'hcount': kk.hcount, 'charge': kk.charge},
                       per_pair={'order': sc.order, 'kekule_order': kk.kekule_order}, per_graph={'kekule_status': kk.status})
    for r, m, p in zip(out, rows, np.split(np.asarray(pos, dtype=np.float64), np.cumsum(sizes, dtype=int)[:-1])):
        r['rows'] = MolRows(pos=p, **m)
    return out


def _run(graphs, options=HY.HydrogenOptions()):
    node, pos, edge, sizes = H.batch_from(graphs)
    res = _result(node, pos, edge, sizes)
    hy = HY.hydrogens(res, options=options)
    torch.cuda.synchronize()
    B, N = len(sizes), sum(sizes)
    assert hy.status.shape == hy.ok.shape == hy.min_contact.shape == (1, B) and hy.counts.shape == (1, B, 8)
    assert hy.h_pos.shape == (1, N, 4, 3) and hy.h_placed.shape == hy.site_shape.shape == (1, N)
    assert (hy.h_pos.dtype, hy.h_placed.dtype, hy.site_shape.dtype, hy.counts.dtype, hy.status.dtype, hy.min_contact.dtype) == (
        torch.float32, torch.uint8, torch.uint8, torch.int32, torch.int32, torch.float32)
    return res, hy, _split(hy, pos.numpy(), sizes)


def _validate(r, options=None, where='', safe_only=False):
    """One graph against the restatement on the device's own inputs; returns the worst error / bound and the restatement.
    safe_only: (None, None) without a comparison if the restatement says a float comparison of this input could flip in fp32."""
    want = H.restate(r['rows'], options)
    if safe_only and not H.is_safe(want, options):
        return None, None
    return H.compare(r, want, r['rows'].pos, options, where=where), want


def _bits(r):
    return {k: bits(r[k]) for k in NAMES}


def _examples_and_mirrors():
    graphs = H.example_graphs()
    return graphs + [(c, b, H.mirrored(p)) for c, b, p in graphs]


def test_examples_by_hand_their_mirror_images_twice_into_recycled_memory():
    graphs, n = _examples_and_mirrors(), len(H.EXAMPLES)
    for clash in H.EXAMPLE_CLASH:
        opt = HY.HydrogenOptions(clash_min=clash, max_contacts=10)
        res, hy, got = _run(graphs, opt)
        for g, r in enumerate(got):
            _validate(r, opt, where='example %d clash %g' % (g, clash))
        for (name, (c, _, _, sites)), r, mr in zip(H.EXAMPLES.items(), got[:n], got[n:]):
            assert {i: (int(r['h_placed'][i]), int(r['site_shape'][i])) for i in range(len(c)) if r['h_placed'][i]} == sites, name
            assert mr['counts'].tolist() == r['counts'].tolist() and mr['status'] == r['status'], name
            assert abs(mr['min_contact'] - r['min_contact']) <= 1e-5 or mr['min_contact'] == r['min_contact'], name
        by = dict(zip(H.EXAMPLES, got[:n]))
        assert by['methane']['counts'].tolist() == [4, 1, 1, 0, 0, 0, 0, 1] and by['methane']['min_contact'] == float('inf')   # four slots
        assert (by['ethane']['counts'][6] == 0) if clash < 1 else (by['ethane']['counts'][6] == 6 + 9 and by['benzene']['status'] & HY.HYD_CONTACTS)
        assert hy.ok[0, list(H.EXAMPLES).index('benzene')].item() == (clash < 1)
        # the outputs do not depend on what their buffers held: a call into recycled memory agrees bit for bit
        first = [_bits(r) for r in got]
        del res, hy, got
        torch.empty(1 << 22, dtype=torch.uint8, device=DEV).fill_(0xEE)
        assert [_bits(r) for r in _run(graphs, opt)[2]] == first


def test_generated_family_against_the_restatement(family):
    _, hy, got = _run(family, FAMILY_OPT)
    ratios = [_validate(r, FAMILY_OPT, where='family %d' % g)[0] for g, r in enumerate(got)]
    print('device, worst error / bound over the family: %.4f' % max(ratios))
    assert 0.0 < max(ratios) <= 1.0
    assert sum(r['status'] == HY.HYD_NO_KEKULE for r in got) == 2 and hy.ok.sum().item() == len(got) - 2
    for r in got:
        if r['status'] == HY.HYD_NO_KEKULE:
            assert not (r['h_pos'].any() or r['h_placed'].any() or r['site_shape'].any() or r['counts'].any()) and r['min_contact'] == 0.0
    assert sum(int(r['counts'][5]) for r in got) >= 20 and sum(int(r['counts'][0]) for r in got) >= 1000


def test_renumbered_graphs(family):
    """Sites with two or more neighbours and no fallback keep the same set of hydrogen positions per parent (a tetrahedral site with two
    neighbours and one hydrogen: one of the set's two); sites with at most one
    depend on the index rule by definition: for them the lengths, the angle to the bond and equality with the restatement hold."""
    graphs = H.example_graphs() + [g for g in family if 3 <= len(g[0]) <= 65][:20]
    node, pos, edge, sizes = H.batch_from(graphs)
    node2, pos2, edge2, perms = _permute_batch(node, pos, edge, sizes, seed=29)
    outs = []
    for nd, ps, ed in ((node, pos, edge), (node2, pos2, edge2)):
        outs.append(_split(HY.hydrogens(_result(nd, ps, ed, sizes), options=FAMILY_OPT), ps.numpy(), sizes))
    same = cone = 0
    for g, (a, b) in enumerate(zip(*outs)):
        _, want_a = _validate(a, FAMILY_OPT, where='numbering %d' % g)
        _, want_b = _validate(b, FAMILY_OPT, where='renumbered %d' % g, safe_only=True)
        if want_b is None:
            continue                                                   # (an argmin that the new numbering decides by less than the margin)
        _, nbrs, _, _, _ = H.graph_of_rows(a['rows'].cls, a['rows'].kekule_order, a['rows'].order)
        p, pa = perms[g], a['rows'].pos
        for i in range(sizes[g]):
            h, shape = int(a['h_placed'][i]), int(a['site_shape'][i])
            assert int(b['h_placed'][p[i]]) == h, (g, i)
            if h and len(nbrs[i]) >= 2 and shape != H.GEN and int(b['site_shape'][p[i]]) != H.GEN:
                assert int(b['site_shape'][p[i]]) == shape, (g, i)
                tol = 2 * max(H.position_bound(np.abs(pa).max(), max(FAMILY_OPT.xh_length), s) for s in want_a['s'][i, :h])
                # (a renumbering may swap u0 and u1: the cross product changes sign and the two slots of a tetrahedral (2, h) site
                # change places; with h = 1 the one hydrogen then stands on the other side of the neighbours' plane)
                mine = [a['h_pos'][i, k].astype(np.float64) for k in range(h)]
                if shape == H.TET and len(nbrs[i]) == 2 and h == 1:
                    nn = np.cross(pa[nbrs[i][0]] - pa[i], pa[nbrs[i][1]] - pa[i])
                    nn = nn / np.linalg.norm(nn)
                    mine.append(mine[0] - 2.0 * float(np.dot(mine[0] - pa[i], nn)) * nn)
                for k in range(h):
                    assert min(np.abs(x - b['h_pos'][p[i], k]).max() for x in mine) <= tol, (g, i, k)
                same += 1
            elif h and len(nbrs[i]) == 1 and shape in (H.TET, H.TRIG):
                want = {H.TET: H.TET_COS, H.TRIG: -0.5}[shape]
                for r, q, at in ((a, pa, i), (b, b['rows'].pos, p[i])):
                    j = H.graph_of_rows(r['rows'].cls, r['rows'].kekule_order, r['rows'].order)[1][at][0]
                    for k in range(h):
                        v, u = r['h_pos'][at, k] - q[at], q[j] - q[at]
                        assert abs(np.linalg.norm(v) - FAMILY_OPT.xh_length[int(r['rows'].cls[at])]) < 1e-5
                        assert abs(float(np.dot(v, u) / (np.linalg.norm(v) * np.linalg.norm(u))) - want) < 1e-5, (g, i, k)
                cone += 1
    assert same >= 100 and cone >= 50


def test_rotation_and_translation_move_the_hydrogens_with_the_molecule(family):
    """On the sites whose rule uses no coordinate axis and no fixed vertex; within the two bounds."""
    graphs = H.example_graphs() + [g for g in family if 3 <= len(g[0]) <= 65][:20]
    c, s = np.cos(0.7), np.sin(0.7)
    rot = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, np.cos(1.9), -np.sin(1.9)], [0, np.sin(1.9), np.cos(1.9)]])
    shift = np.array([3.0, -2.0, 1.0])
    moved = [(cl, b, (np.asarray(p, dtype=np.float64) @ rot.T + shift).astype(np.float32)) for cl, b, p in graphs]
    _, _, before = _run(graphs, FAMILY_OPT)
    _, _, after = _run(moved, FAMILY_OPT)
    held = 0
    for g, (a, b) in enumerate(zip(before, after)):
        _, wa = _validate(a, FAMILY_OPT, where='before %d' % g)
        _, wb = _validate(b, FAMILY_OPT, where='after %d' % g, safe_only=True)
        if wb is None:
            continue                                                   # (the rotation brought an axis or vertex choice within the margin)
        _, nbrs, _, _, _ = H.graph_of_rows(a['rows'].cls, a['rows'].kekule_order, a['rows'].order)
        pa, pb = a['rows'].pos, b['rows'].pos
        for i in range(len(pa)):
            h = int(a['h_placed'][i])
            axis_free = len(nbrs[i]) >= 2 or (len(nbrs[i]) == 1 and len(nbrs[nbrs[i][0]]) >= 2)
            if not h or not axis_free or a['site_shape'][i] == H.GEN or b['site_shape'][i] == H.GEN:
                continue
            assert a['site_shape'][i] == b['site_shape'][i] and b['h_placed'][i] == h
            for k in range(h):
                # the moved fp32 coordinates are a rounding of the exact image: the restatement's own two answers differ by that much
                slack = np.abs(wb['h_pos'][i, k] - (wa['h_pos'][i, k] @ rot.T + shift)).max()
                tol = (H.position_bound(np.abs(pa).max(), max(FAMILY_OPT.xh_length), wa['s'][i, k])
                       + H.position_bound(np.abs(pb).max(), max(FAMILY_OPT.xh_length), wb['s'][i, k]) + slack)
                assert np.abs(b['h_pos'][i, k] - (a['h_pos'][i, k].astype(np.float64) @ rot.T + shift)).max() <= tol, (g, i, k)
            held += 1
    assert held >= 150


def test_alone_and_inside_a_batch_bit_identical(family):
    pick = [g for g in range(len(family)) if len(family[g][0]) in (1, 2, 64, 65, 128)][:10]
    assert {len(family[g][0]) for g in pick} == {1, 2, 64, 65, 128}      # the lane-ownership boundaries and PG_MOL_MAX_ATOMS
    _, _, together = _run([family[g] for g in pick], FAMILY_OPT)
    for g, r in zip(pick, together):
        _, _, (alone,) = _run([family[g]], FAMILY_OPT)
        assert _bits(alone) == _bits(r), g
        assert all(np.array_equal(x, y) for x, y in zip(alone['rows'], r['rows'])), g


def test_trajectory_frames_in_one_launch():
    """frames='traj', F = 2 in one launch over strided frames: ethane and acetamide, then their mirror images."""
    g = {k: H.EXAMPLES[k][:3] for k in ('ethane', 'acetamide')}
    frames = [[g['ethane'], g['acetamide']], [(g['ethane'][0], g['ethane'][1], H.mirrored(np.array(g['ethane'][2]))),
                                              (g['acetamide'][0], g['acetamide'][1], H.mirrored(np.array(g['acetamide'][2])))]]
    per = [H.batch_from(f) for f in frames]
    sizes = per[0][3]
    traj = tuple(torch.stack([p[k] for p in per]).to(DEV) for k in range(3))
    res = _result(*per[-1][:3], sizes, traj=traj)
    opt = HY.HydrogenOptions(clash_min=0.4)
    hy = HY.hydrogens(res, frames='traj', options=opt)
    assert hy.status.shape == (2, 2) and hy.h_pos.shape == (2, 6, 4, 3) and hy.ok.all()
    for f in range(2):
        for k, r in enumerate(_split(hy, per[f][1].numpy(), sizes, f)):
            _validate(r, opt, where='frame %d graph %d' % (f, k))
    final = HY.hydrogens(res, options=opt)
    assert all(torch.equal(getattr(final, k)[0], getattr(hy, k)[1]) for k in NAMES) and final.kekule is not hy.kekule
    again = HY.hydrogens(res, frames='traj', screen=hy.screen, kekule=hy.kekule, options=opt)
    assert again.screen is hy.screen and again.kekule is hy.kekule and all(torch.equal(getattr(again, k), getattr(hy, k)) for k in NAMES)
    with pytest.raises(ValueError, match='screen'):
        HY.hydrogens(res, frames='final', kekule=hy.kekule)
    with pytest.raises(ValueError, match='HydrogenOptions'):
        HY.hydrogens(res, options=M.StereoLimits())
    with pytest.raises(ValueError, match='kekule= must be a Kekule'):
        HY.hydrogens(res, kekule=hy.screen)


def test_smallest_shapes_that_can_go_wrong():
    c, b, p, _ = H.EXAMPLES['propane']
    nan = np.array(p, dtype=np.float32)
    nan[0, 1] = np.nan
    dropped = ([c[0], 11, c[1], c[2]], {(0, 2): 1, (2, 3): 1, (0, 1): 1}, np.array([p[0], [9.0, 9.0, 9.0], p[1], p[2]], dtype=np.float32))
    five = ([1] * 5, {(i, (i + 1) % 5) if i < 4 else (0, 4): 4 for i in range(5)}, np.array(H._ring(5, 1.4), dtype=np.float32))
    empty = ([], {}, np.zeros((0, 3), dtype=np.float32))
    graphs = [(c, b, nan), dropped, empty, H.example_graphs()[0], five, (c, b, np.array(p, dtype=np.float32))]
    opt = HY.HydrogenOptions(clash_min=0.4)
    _, hy, got = _run(graphs, opt)
    for g, r in enumerate(got):
        _validate(r, opt, where='graph %d' % g)
    assert got[0]['status'] == HY.HYD_NONFINITE | HY.HYD_GENERIC | HY.HYD_HAS_HYDROGEN and got[0]['h_placed'].tolist() == [0, 0, 3]
    assert got[1]['h_placed'].tolist() == [3, 0, 2, 3] and got[1]['counts'][7] == 3      # compact against local index
    assert np.array_equal(got[1]['h_pos'][[0, 2, 3]], got[5]['h_pos'])                    # a dropped atom has no influence
    assert got[2]['status'] == 0 and not got[2]['counts'].any() and got[2]['min_contact'] == float('inf')
    assert got[3]['h_placed'].tolist() == [4] and got[4]['status'] == HY.HYD_NO_KEKULE
    assert hy.ok.tolist() == [[False, True, True, True, False, True]]


def test_too_many_oversize_and_cpu_results_are_refused():
    n = M.MAX_ATOMS + 1
    h = n * (n - 1) // 2

    class Rows:
        def __init__(self, n, h, hcount=0):
            self.cls = self.charge = torch.ones(1, n, dtype=torch.int8, device=DEV)
            self.order = self.kekule_order = torch.zeros(1, h, dtype=torch.int8, device=DEV)
            self.hcount = torch.full((1, n), hcount, dtype=torch.uint8, device=DEV)
            self.status = torch.zeros(1, 1, dtype=torch.int32, device=DEV)
            self.lig_off = torch.tensor([0, n], dtype=torch.int32, device=DEV)
            self.bond_off = torch.tensor([0, 2 * h], dtype=torch.int32, device=DEV)
    full = lambda shape, dt: torch.full(shape, 77, dtype=dt, device=DEV)   # noqa: E731
    outs = lambda n: dict(status=full((1, 1), torch.int32), counts=full((1, 1, 8), torch.int32), h_pos=full((1, n, 4, 3), torch.float32),   # noqa: E731
                          h_placed=full((1, n), torch.uint8), site_shape=full((1, n), torch.uint8), min_contact=full((1, 1), torch.float32))
    rows, out, pos = Rows(n, h), outs(n), torch.zeros(n, 3, device=DEV)
    opt = HY.HydrogenOptions()
    table = HY._length_table(opt, pos.device)
    with pytest.raises(RuntimeError) as err:
        HY._launch_hydrogens(hip.lib(), pos, 0, rows, rows, 1, 1, n, table, opt, out)
    assert 'PG_MOL_MAX_ATOMS' in str(err.value) and 'pg_mol_hydrogens' in str(err.value) and str(n) in str(err.value)
    with pytest.raises(RuntimeError, match='pg_mol_hydrogens'):
        HY._launch_hydrogens(hip.lib(), pos, 0, rows, rows, 1, 1, -1, table, opt, out)
    with pytest.raises(ValueError, match='hydrogens'):
        HY._launch_hydrogens(hip.lib(), pos[:5], 0, rows, rows, 1, 1, n, table, opt, out)
    torch.cuda.synchronize()
    assert all((t == 77).all() for t in out.values())
    # five hydrogens on one atom (no shipped table gives that): nothing is placed in the graph
    rows, out, pos = Rows(3, 3, hcount=5), outs(3), torch.tensor([[0.0, 0, 0], [3.0, 0, 0], [0, 3.0, 0]], device=DEV)
    HY._launch_hydrogens(hip.lib(), pos, 0, rows, rows, 1, 1, 3, table, opt, out)
    torch.cuda.synchronize()
    assert out['status'].item() == HY.HYD_TOO_MANY and out['counts'].flatten().tolist() == [0] * 7 + [3]
    assert not out['h_pos'].any() and not out['h_placed'].any() and not out['site_shape'].any() and out['min_contact'].item() == float('inf')
    node, p, edge, sizes = H.batch_from(H.example_graphs()[:2])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        HY.hydrogens(_result(node, p, edge, sizes, dev='cpu'))
    res = _result(torch.zeros(0, 12), torch.zeros(0, 3), torch.zeros(0, 6), [])       # an empty batch returns without a launch
    assert HY.hydrogens(res).h_pos.shape == (1, 0, 4, 3)


def _read_block(text):
    """(element symbols, bonds) of a V2000 block."""
    atoms, bonds = read_mol_block(text)
    return [a[0] for a in atoms], bonds


def test_assemble_sdf_sample_valid_and_cli_carry_the_hydrogens(tmp_path):
    names = ['acetamide', 'benzene', 'tetramethylammonium']
    graphs = [H.EXAMPLES[k][:3] for k in names]
    res, hy, got = _run(graphs, HY.HydrogenOptions(clash_min=0.4))
    plain, full = M.assemble(res), M.assemble(res, kekule=hy.kekule, hydrogens=hy)
    for g, (p, m, r) in enumerate(zip(plain, full, got)):
        assert set(m) == set(p) | {'kekule', 'hydrogens'}
        e = m['hydrogens']
        assert set(e) == {'status', 'hydrogens_ok', 'min_contact', 'h_pos', 'h_parent', 'site_shape'} | set(HY.HYD_COUNTS)
        assert e['status'] == r['status'] and [e[k] for k in HY.HYD_COUNTS] == r['counts'].tolist() and e['hydrogens_ok']
        assert e['h_pos'].shape == (e['hydrogens'], 3) and e['h_parent'].tolist() == np.repeat(np.arange(len(r['h_placed'])), r['h_placed']).tolist()
        assert np.array_equal(e['h_pos'], r['h_pos'][r['h_placed'][:, None] > np.arange(4)[None, :]]) and e['site_shape'].tolist() == r['site_shape'].tolist()
        assert e['hydrogens'] == m['kekule']['hydrogens'] == int(m['kekule']['hcount'].sum())
        symbols, bonds = _read_block(M.mol_block(m))
        assert symbols.count('H') == e['hydrogens'] and len(bonds) == len(m['bond_type']) + e['hydrogens']
        assert M.mol_block(p) == M.mol_block({k: v for k, v in m.items() if k not in ('kekule', 'hydrogens')})
    with pytest.raises(ValueError, match='hydrogens='):                 # of another result
        M.assemble(res, kekule=hy.kekule, hydrogens=HY.hydrogens(_result(*H.batch_from(graphs[:1])[:3], [4])))
    path = tmp_path / 'h.sdf'
    M.write_sdf(str(path), full)
    assert path.read_text().count('> <PHOREGEN_HYDROGENS>\nstatus 0x20\n') == 3
    # sample_valid: a stand-in model that hands the three out in turn; max_contacts = 0 at a huge clash_min fails everything
    parts = [H.batch_from([g]) for g in graphs]

    class Rota:
        i = 0

        def sample(self, data, n, device, **kw):
            pick = [parts[(self.i + j) % 3] for j in range(n)]
            self.i += n
            return _result(*(torch.cat([p[k] for p in pick]) for k in range(3)), [p[3][0] for p in pick])
    out = M.sample_valid(Rota(), None, num_samples=3, batch_size=3, hydrogens=True)
    assert len(out['finished']) == 3 and all(m['hydrogens']['hydrogens_ok'] and m['kekule']['kekule_ok'] for m in out['finished'])
    assert [_read_block(M.mol_block(m))[0].count('H') for m in out['finished']] == [5, 6, 12]
    out = M.sample_valid(Rota(), None, num_samples=2, batch_size=3, hydrogens=HY.HydrogenOptions(clash_min=16.0, max_contacts=0), max_failed_factor=1)
    assert not out['finished'] and all(m['hydrogens']['status'] & HY.HYD_CONTACTS for m in out['failed'])
    assert 'hydrogens' not in M.sample_valid(Rota(), None, num_samples=1, batch_size=1)['finished'][0]
    # the command-line tool, a 3-sample run: all-atom blocks whose hydrogens match PHOREGEN_KEKULE's count
    lst = tmp_path / 'files.json'
    lst.write_text(json.dumps([os.path.join(ROOT, 'tests', 'data', 'synthetic_test.phore')]))
    outdir = tmp_path / 'out'
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'sample_cli.py'), '--phore_file_list', str(lst), '--num_samples', '3',
                          '--batch_size', '3', '--outdir', str(outdir), '--kekule', '--hydrogens', '--sdf', '--num_steps', '10',
                          '--hydrogen_options', '{"clash_min": 0.5}'], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    done = torch.load(str(next(outdir.glob('*.pt'))), weights_only=False)
    sdfs = sorted((outdir / 'sdf_results').glob('*.sdf'))
    assert len(sdfs) == len(done) and all(m['hydrogens']['hydrogens_ok'] for m in done)
    for m, path in zip(done, sdfs):
        text = path.read_text()
        symbols, _ = _read_block(text)
        assert 'hydrogens %d\n' % symbols.count('H') in text.split('> <PHOREGEN_KEKULE>')[1].split('> <')[0]
        assert '> <PHOREGEN_HYDROGENS>' in text and symbols.count('H') == m['hydrogens']['hydrogens'] == m['kekule']['hydrogens']
