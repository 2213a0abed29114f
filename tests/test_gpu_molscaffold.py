"""-m gpu: the scaffold kernel (csrc/mol_scaffold.hip through phoregen_amd/scaffold.py) against the plain restatement of
tests/scaffold_reference.py, for all four option pairs, and the analyses that run on the scaffold screen unchanged.  Integer work only:
every comparison is `==` on every output array."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scaffold_reference as S
import smiles_reference as T
from mol_support import C_, CL_, N_, O_, batch_from, cycle, mol_dict, mol_result as _result, permute_batch, rows_of, split_frame
from phoregen_amd import hip
from phoregen_amd import molecule as M
from phoregen_amd import scaffold as SC
from test_molscaffold_host import BY_HAND, BY_HAND_PLAIN

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCREEN_ARRAYS = ('status', 'counts', 'valid', 'cls', 'compact', 'valence2', 'comp', 'order')


def _split(sf, sizes, f=0):
    """Frame f of a `Scaffolds` as one dict of numpy arrays per graph, in the restatement's form."""
    s = sf.screen
    return split_frame(sizes, f, per_atom={'part': sf.part, 'cls': s.cls, 'compact': s.compact, 'valence2': s.valence2, 'comp': s.comp},
                       per_pair={'order': s.order}, per_graph={'counts': sf.counts, 's_counts': s.counts, 'status': s.status, 'valid': s.valid})


def _same(got, want, where=''):
    assert len(got) == len(want)
    for g, (a, b) in enumerate(zip(got, want)):
        assert a['counts'].tolist() == b['counts'].tolist(), (where, g, dict(zip(SC.SCAFFOLD_COUNTS, zip(a['counts'].tolist(), b['counts'].tolist()))))
        assert a['s_counts'].tolist() == b['s_counts'].tolist() and a['status'] == b['status'] and a['valid'] == b['valid'], (where, g)
        for k in ('part', 'cls', 'compact', 'valence2', 'comp', 'order'):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (where, g, k, np.nonzero(a[k] != b[k])[0][:8])


def _check(graphs, where=''):
    """The kernel on one frame == the restatement, for all four option pairs; returns ({options: Scaffolds}, sizes, the source screen)."""
    node, pos, edge, sizes = batch_from(graphs)
    sc = M.screen(_result(node, pos, edge, sizes))
    rows = [rows_of(g[0], g[1]) for g in graphs]
    src = split_frame(sizes, 0, per_atom={'cls': sc.cls}, per_pair={'order': sc.order})
    assert all(np.array_equal(a['cls'], c) and np.array_equal(a['order'], o) for a, (c, o) in zip(src, rows))
    N, H, B = sum(sizes), sum(n * (n - 1) // 2 for n in sizes), len(sizes)
    out = {}
    for exo, gen in S.OPTIONS:
        options = SC.ScaffoldOptions(exocyclic=exo, generic=gen)
        sf = SC.scaffolds(sc, options)
        torch.cuda.synchronize()
        s = sf.screen
        assert sf.source is sc and sf.options == options and isinstance(s, M.Screen) and s.agree is None and s.bonds == sc.bonds
        assert s.num_atoms == sizes and torch.equal(s.lig_off, sc.lig_off) and torch.equal(s.bond_off, sc.bond_off)
        assert sf.part.shape == s.cls.shape == s.compact.shape == s.valence2.shape == s.comp.shape == (1, N) and s.order.shape == (1, H)
        assert sf.counts.shape == (1, B, 8) and s.counts.shape == (1, B, 4) and s.status.shape == s.valid.shape == (1, B)
        assert (sf.part.dtype, sf.counts.dtype, s.status.dtype, s.counts.dtype, s.valid.dtype) == (torch.uint8, torch.int32, torch.int32,
                                                                                                    torch.int32, torch.bool)
        assert (s.cls.dtype, s.compact.dtype, s.valence2.dtype, s.comp.dtype, s.order.dtype) == (torch.int8, torch.int16, torch.uint8,
                                                                                                  torch.int16, torch.int8)
        _same(_split(sf, sizes), [S.scaffold_of_rows(c, o, exo, gen) for c, o in rows], '%s exocyclic=%s generic=%s' % (where, exo, gen))
        out[(exo, gen)] = sf
    return out, sizes, sc


def _equal_screens(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in SCREEN_ARRAYS)


def test_named_molecules_by_hand_and_by_the_restatement():
    names = list(S.NAMED)
    got, sizes, sc = _check([S.NAMED[k] for k in names], 'named')
    assert sizes[:6] == [0, 1, 2, 3, 128, 128]
    for exo in (True, False):
        hand = BY_HAND if exo else {**BY_HAND, **BY_HAND_PLAIN}
        for k, r in zip(names, _split(got[(exo, False)], sizes)):
            assert r['part'].tolist() == hand[k][0] and r['counts'].tolist() == hand[k][2], (k, exo)
    status = dict(zip(names, got[(True, False)].screen.status[0].tolist()))
    assert status['two_ring_systems'] == M.STATUS_DISCONNECTED and status['chain128'] == status['none'] == M.STATUS_NO_ATOMS
    assert status['ring3_tail125'] == status['linker_carbonyl'] == 0
    src = dict(zip(names, sc.status[0].tolist()))
    assert src['dropped_in_ring'] & M.STATUS_HAD_MASKED_ATOM and src['absorbing_on_ring'] & M.STATUS_HAD_ABSORBING_BOND
    # the outputs do not depend on what their buffers held: a call into recycled memory agrees
    first = got[(True, False)]
    again = SC.scaffolds(sc)
    assert _equal_screens(first.screen, again.screen) and torch.equal(first.part, again.part) and torch.equal(first.counts, again.counts)


def test_word_and_lane_boundaries_on_the_family():
    graphs, wants = S.family()
    assert sorted({len(g[0]) for g in graphs if len(g[0]) >= 63}) == list(S.FAMILY_SIZES)
    got, sizes, _ = _check(graphs, 'family')
    placed = {b: set() for b in S.BOUNDARY}
    for r, want in zip(_split(got[(True, False)], sizes), wants):
        for i, role in want.items():
            assert r['part'][i] == role
            placed[i].add(role)
    assert all(roles == set(S.ROLES) for roles in placed.values()), placed      # every boundary index has held every part


def test_trajectory_frames_strided():
    """frames='traj', F = 3 in one launch on tensors whose frames are not dense: every frame equals its own single-frame run."""
    names = [['toluene', 'linker_carbonyl', 'spiro'], ['benzene', 'diphenylmethane_methyl', 'fused'], ['ring_carbonyl', 'biphenyl', 'bridged']]
    pad = (7, 14, 10)
    frames = []
    for row in names:                                                  # the graphs of a frame padded with lone atoms to one size each
        graphs = []
        for k, n in zip(row, pad):
            classes, bonds = S.NAMED[k]
            graphs.append((list(classes) + [O_] * (n - len(classes)), bonds))
        frames.append(graphs)
    per = [batch_from(f) for f in frames]
    sizes = per[0][3]
    assert all(p[3] == sizes for p in per) and sizes == [7, 14, 10]
    traj = []
    for k in range(3):
        rows, width = per[0][k].shape
        big = torch.full((3, rows + 4, width), 0.5, device=DEV)
        big[:, :rows] = torch.stack([p[k] for p in per]).to(DEV)
        traj.append(big[:, :rows])
        assert not traj[-1].is_contiguous() and traj[-1][0].is_contiguous()
    res = _result(*per[-1][:3], sizes, traj=tuple(traj))
    for exo, gen in S.OPTIONS:
        options = SC.ScaffoldOptions(exo, gen)
        sf = SC.scaffolds(M.screen(res, frames='traj'), options)
        assert sf.part.shape == (3, 31) and sf.counts.shape == (3, 3, 8) and sf.screen.order.shape == (3, 21 + 91 + 45)
        for f, (p, graphs) in enumerate(zip(per, frames)):
            _same(_split(sf, sizes, f), S.scaffold_of_graphs(graphs, exo, gen), 'frame %d' % f)
            alone = SC.scaffolds(M.screen(_result(*p[:3], sizes)), options)
            assert all(torch.equal(getattr(sf.screen, k)[f], getattr(alone.screen, k)[0]) for k in SCREEN_ARRAYS)
            assert torch.equal(sf.part[f], alone.part[0]) and torch.equal(sf.counts[f], alone.counts[0])
    assert sf.counts[:, 1, 0].tolist() == [13, 13, 12]                  # (generic frameworks of benzophenone, the diphenylmethane, biphenyl)


def test_renumbered_batch():
    graphs, _ = S.family()
    graphs = graphs[::2] + [S.NAMED['linker_carbonyl'], S.NAMED['two_ring_systems'], S.NAMED['dropped_in_ring']]
    node, pos, edge, sizes = batch_from(graphs)
    node2, pos2, edge2, perms = permute_batch(node, pos, edge, sizes, seed=11)
    sc, sc2 = M.screen(_result(node, pos, edge, sizes)), M.screen(_result(node2, pos2, edge2, sizes))
    for exo, gen in S.OPTIONS:
        options = SC.ScaffoldOptions(exo, gen)
        a, b = SC.scaffolds(sc, options), SC.scaffolds(sc2, options)
        assert torch.equal(a.counts, b.counts) and torch.equal(a.screen.counts, b.screen.counts) and torch.equal(a.screen.status, b.screen.status)
        for g, (x, y, p) in enumerate(zip(_split(a, sizes), _split(b, sizes), perms)):
            for k in ('part', 'cls', 'valence2'):
                assert y[k][p].tolist() == x[k].tolist(), (g, k)
        keys = SC.scaffold_keys(a).key
        assert torch.equal(keys, SC.scaffold_keys(b).key) and (gen or len(set(keys[0].tolist())) > 5)
        fa, fb = M.fingerprints(a.screen), M.fingerprints(b.screen)
        assert torch.equal(fa.fp, fb.fp) and torch.equal(fa.bits, fb.bits)


def test_scaffold_of_a_scaffold():
    graphs, _ = S.family()
    graphs = graphs + list(S.NAMED.values())
    got, sizes, _ = _check(graphs, 'first pass')
    for exo, gen in ((True, False), (False, False), (False, True)):
        sf = got[(exo, gen)]
        again = SC.scaffolds(sf.screen, sf.options)
        assert _equal_screens(again.screen, sf.screen)
        assert set(again.part.unique().tolist()) <= {0, 2, 3, 4} and torch.equal(again.part == 0, sf.part <= 1)
        assert torch.equal(again.part[sf.part >= 2], sf.part[sf.part >= 2]) and (again.counts[..., 5] == 0).all()
    # generic with exocyclic does not reproduce itself: the former exocyclic atoms are single-bonded by then and go
    sf = got[(True, True)]
    again = SC.scaffolds(sf.screen, sf.options)
    assert (sf.counts[..., 4] > 0).any() and (again.counts[..., 4] == 0).all()
    assert torch.equal(again.counts[..., 0], sf.counts[..., 0] - sf.counts[..., 4]) and torch.equal(again.counts[..., 5], sf.counts[..., 4])
    assert _equal_screens(again.screen, got[(False, True)].screen)


def _mol_of_text(text):
    atoms, bonds = T.read_smiles(text)
    return mol_dict([z for z, _, _ in atoms], list(bonds), list(bonds.values()))


def test_composition_with_keys_smiles_assemble_and_groups():
    names = ['benzene', 'toluene', 'chlorobenzene', 'pyridine', 'picoline', 'linker_carbonyl', 'thiobenzophenone', 'hexane']
    pyridine = ([N_] + [C_] * 5, cycle(6, 4))
    thio = (S.NAMED['linker_carbonyl'][0][:13] + [S.S_], S.NAMED['linker_carbonyl'][1])
    graphs = [S.NAMED['benzene'], S.NAMED['toluene'], ([C_] * 6 + [CL_], S.NAMED['toluene'][1]), pyridine,
              (pyridine[0] + [C_], {**pyridine[1], (2, 6): 1}), S.NAMED['linker_carbonyl'], thio, ([C_] * 6, S.chain(6, 1))]
    node, pos, edge, sizes = batch_from(graphs)
    res = _result(node, pos, edge, sizes)
    sc = M.screen(res)
    sf, fw = SC.scaffolds(sc), SC.scaffolds(sc, SC.ScaffoldOptions(generic=True))
    key, fkey = SC.scaffold_keys(sf).key[0], SC.scaffold_keys(fw).key[0]
    src_key = M.molecule_keys(sc).key[0].tolist()
    # scaffold identity: decorations do not matter, ring heteroatoms do; the scaffold of benzene is benzene
    k = dict(zip(names, key.tolist()))
    assert k['benzene'] == k['toluene'] == k['chlorobenzene'] == src_key[0] and k['pyridine'] == k['picoline'] == src_key[3]
    assert k['benzene'] != k['pyridine'] and k['linker_carbonyl'] != k['thiobenzophenone'] and len(set(src_key)) == len(names)
    assert k['hexane'] & S.MS.M64 == M.KEY_EMPTY
    # frameworks coincide where only heteroatoms (and bond orders) differ
    fk = dict(zip(names, fkey.tolist()))
    assert fk['benzene'] == fk['pyridine'] == fk['picoline'] and fk['linker_carbonyl'] == fk['thiobenzophenone'] != fk['benzene']
    # groups by key, and confirmed on the scaffold molecules
    group, size = SC.scaffold_groups(key)
    assert group.tolist() == [0, 0, 0, 3, 3, 5, 6, 7] and size.tolist() == [3, 3, 3, 2, 2, 1, 1, 1] and group.device == key.device
    mols = M.assemble(res, screen=sf.screen)
    exact, _ = SC.scaffold_groups(key, mols)
    assert torch.equal(exact, group)
    assert SC.pick_per_scaffold(group, 1).tolist() == [0, 3, 5, 6, 7] and SC.pick_per_scaffold(group, 2).tolist() == [0, 1, 3, 4, 5, 6, 7]
    fgroup, fsize = SC.scaffold_groups(fkey)
    assert fgroup.tolist() == [0, 0, 0, 0, 0, 5, 5, 7] and fsize.max().item() == 5
    # the scaffold molecules: toluene's is benzene, atom for atom; hexane's is empty
    plain = M.assemble(res)
    assert M.same_molecule(mols[1], plain[0]) and M.same_molecule(mols[2], plain[0]) and not M.same_molecule(mols[1], plain[1])
    assert mols[1]['element'] == [6] * 6 and mols[2]['element'] == [6] * 6 and mols[7]['element'] == [] and not mols[7]['valid']
    assert mols[5]['element'] == [6] * 13 + [8] and M.same_molecule(mols[5], plain[5])
    # scaffold SMILES: written from the scaffold screen, it reads back as the scaffold -- toluene's as benzene's own text does
    text = M.smiles(res, screen=sf.screen)
    assert text.screen is sf.screen and text.ok[0].tolist() == [True] * 8
    strings, own = text.strings(), M.smiles(res, screen=sc).strings()
    assert strings[7] == '' and int(text.status[0, 7]) & M.SMILES_EMPTY
    assert M.same_molecule(_mol_of_text(strings[1]), _mol_of_text(own[0])) and len(T.read_smiles(strings[1])[0]) == 6
    assert M.same_molecule(_mol_of_text(strings[2]), _mol_of_text(strings[0])) and not M.same_molecule(_mol_of_text(own[1]), _mol_of_text(own[0]))
    atoms, bonds = T.read_smiles(strings[5])
    assert sorted(z for z, _, _ in atoms) == [6] * 13 + [8] and len(bonds) == 15 and sum(o == 2 for o in bonds.values()) == 7
    # batch_of: finished molecules back on the device give the same screen rows and the same scaffolds
    back = SC.batch_of(plain, DEV)
    sc2 = M.screen(back)
    assert torch.equal(sc2.cls, sc.cls) and torch.equal(sc2.order, sc.order) and sc2.num_atoms == sizes
    assert torch.equal(SC.scaffold_keys(SC.scaffolds(sc2)).key[0], key)
    # similarity of scaffolds: equal scaffolds have equal fingerprints, whatever the decoration
    fp = M.fingerprints(sf.screen).fp[0]
    assert torch.equal(fp[0], fp[1]) and torch.equal(fp[0], fp[2]) and not torch.equal(fp[0], fp[3]) and not fp[7].any()


def test_cpu_screen_and_oversize_graph_are_refused():
    n = M.MAX_ATOMS + 1
    h = n * (n - 1) // 2
    cls = torch.zeros(1, n, dtype=torch.int8, device=DEV)
    order = torch.zeros(1, h, dtype=torch.int8, device=DEV)
    off = torch.tensor([0, n], dtype=torch.int32, device=DEV)
    boff = torch.tensor([0, 2 * h], dtype=torch.int32, device=DEV)
    full = lambda shape, dt: torch.full(shape, 77, dtype=dt, device=DEV)   # noqa: E731
    part, counts = full((1, n), torch.uint8), full((1, 1, 8), torch.int32)
    out = dict(status=full((1, 1), torch.int32), counts=full((1, 1, 4), torch.int32), cls=full((1, n), torch.int8),
               compact=full((1, n), torch.int16), valence2=full((1, n), torch.uint8), comp=full((1, n), torch.int16),
               order=full((1, h), torch.int8))
    with pytest.raises(RuntimeError) as err:
        SC._launch_scaffold(hip.lib(), cls, order, off, boff, 1, 1, n, 1, part, counts, out)
    assert 'PG_MOL_MAX_ATOMS' in str(err.value) and 'pg_mol_scaffold' in str(err.value) and str(n) in str(err.value)
    with pytest.raises(RuntimeError, match='pg_mol_scaffold: flags 4'):
        SC._launch_scaffold(hip.lib(), cls, order, off, boff, 1, 1, 8, 4, part, counts, out)
    with pytest.raises(ValueError, match='do not fit'):
        SC._launch_scaffold(hip.lib(), cls, order, off, boff, 1, 1, 8, 1, part[:, :5].contiguous(), counts, out)
    torch.cuda.synchronize()
    assert all((t == 77).all() for t in [part, counts, *out.values()])
    sc = M.Screen(status=out['status'], counts=out['counts'], valid=out['status'] == 0, cls=cls, compact=out['compact'],
                  valence2=out['valence2'], comp=out['comp'], order=order, lig_off=off, bond_off=boff, num_atoms=[n])
    with pytest.raises(RuntimeError, match='PG_MOL_MAX_ATOMS'):
        SC.scaffolds(sc)
    on_cpu = M.Screen(**{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in vars(sc).items()})
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        SC.scaffolds(on_cpu)
    # empty batches return without a launch
    empty = SC.scaffolds(M.screen(_result(torch.zeros(0, 12), torch.zeros(0, 3), torch.zeros(0, 6), [])))
    assert empty.part.shape == (1, 0) and empty.counts.shape == (1, 0, 8) and empty.screen.order.shape == (1, 0)


def test_sample_cli_writes_the_scaffold_files(tmp_path):
    lst = tmp_path / 'files.json'
    lst.write_text(json.dumps([os.path.join(ROOT, 'tests', 'data', 'synthetic_test.phore')]))
    out = tmp_path / 'out'
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'sample_cli.py'), '--phore_file_list', str(lst), '--num_samples', '3',
                          '--batch_size', '3', '--outdir', str(out), '--scaffolds', '--max_per_scaffold', '1', '--num_steps', '10'],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    done = torch.load(str(next(out.glob('*.pt'))), weights_only=False)
    (path,) = out.glob('*_scaffolds.txt')
    lines = [ln.split() for ln in path.read_text().split('\n')[:-1]]
    assert len(lines) == len(done) and all(len(ln) == 7 for ln in lines)
    assert [int(ln[0]) for ln in lines] == list(range(len(done)))
    assert all(len(ln[1]) == 16 and len(ln[2]) == 16 and int(ln[1], 16) >= 0 and int(ln[2], 16) >= 0 for ln in lines)
    groups = [int(ln[3]) for ln in lines]
    first = {}
    for i, ln in enumerate(lines):                                     # the group is the first row with the line's scaffold key
        assert groups[i] == first.setdefault(ln[1], i)
    # the figures are those of the finished molecules, computed again here
    sf = SC.scaffolds(M.screen(SC.batch_of(done, DEV)))
    key = SC.scaffold_keys(sf).key[0].tolist()
    assert [ln[1] for ln in lines] == ['%016x' % (k & (1 << 64) - 1) for k in key]
    assert [[int(ln[4]), int(ln[5])] for ln in lines] == sf.counts[0][:, [0, 6]].tolist()
    for ln, n_atoms in zip(lines, sf.counts[0, :, 0].tolist()):
        if n_atoms == 0:
            assert ln[6] == '-' and int(ln[1], 16) == M.KEY_EMPTY
        elif ln[6] != '-':
            assert len(T.read_smiles(ln[6])[0]) == n_atoms
    (path,) = out.glob('*_scaffold_summary.txt')
    summary = dict(ln.split(': ') for ln in path.read_text().split('\n')[:-1])
    assert set(summary) == {'molecules', 'distinct_scaffolds', 'distinct_frameworks', 'without_scaffold', 'largest_group'}
    assert int(summary['molecules']) == len(done) and int(summary['distinct_scaffolds']) == len(set(groups))
    assert int(summary['distinct_frameworks']) == len({ln[2] for ln in lines}) <= int(summary['distinct_scaffolds'])
    assert int(summary['without_scaffold']) == sum(ln[6] == '-' and int(ln[4]) == 0 for ln in lines)
    assert int(summary['largest_group']) == max([groups.count(g) for g in set(groups)], default=0)
    (path,) = out.glob('*_scaffold_picks.txt')
    picks = [int(ln) for ln in path.read_text().split('\n')[:-1]]
    assert picks == sorted(set(groups))
