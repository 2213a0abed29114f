"""From sampler output to molecules (beyond the reference's library code; its driver does this with RDKit, sample_all.py:79-175).

`screen` answers, on the device and for every (frame, graph) in one launch (csrc/mol_screen.hip), the two questions the top-up loop
of sample_all.py needs: is this ONE molecule, and can these atoms carry these bonds.  `assemble` turns the final prediction into
per-molecule arrays with `decode_data`'s keys, `mol_block` / `write_sdf` write them as V2000 mol blocks, `sample_valid` is the loop
that samples until enough molecules have passed.  No RDKit, no OpenBabel: `valid` is necessary, not sufficient, for the reference's
`Chem.SanitizeMol` (DESIGN.md "From sampler output to molecules")."""
from dataclasses import dataclass

import numpy as np
import torch

from . import hip
from .utils.sample_utils import ATOM_TYPES

STATUS_NO_ATOMS = 1              # nothing kept
STATUS_DISCONNECTED = 2          # more than one connected component (the heavy-atom equivalent of `'.' in smiles`)
STATUS_VALENCE = 4               # an atom above MAX_VALENCE (+ 1/2 if it has an aromatic bond)
STATUS_NONFINITE = 8             # a kept atom with a non-finite coordinate
STATUS_HAD_MASKED_ATOM = 16      # informational: an atom of class 11 was dropped
STATUS_HAD_ABSORBING_BOND = 32   # informational: a bond row (a < b) of class 5, read as "no bond"
FAIL_MASK = STATUS_NO_ATOMS | STATUS_DISCONNECTED | STATUS_VALENCE | STATUS_NONFINITE
STATUS_NAMES = {STATUS_NO_ATOMS: 'NO_ATOMS', STATUS_DISCONNECTED: 'DISCONNECTED', STATUS_VALENCE: 'VALENCE',
                STATUS_NONFINITE: 'NONFINITE', STATUS_HAD_MASKED_ATOM: 'HAD_MASKED_ATOM',
                STATUS_HAD_ABSORBING_BOND: 'HAD_ABSORBING_BOND'}

# Largest explicit valence an atom may carry, by atomic number: the largest entry of each element's default valence list as RDKit has
# it, with N raised to 4 because the reference turns a four-valent N into N+ instead of failing (utils/sample_utils.py:437-440).
# CAVEAT: written from memory; RDKit is not a dependency of this project and the table has not been checked against it.  The rule is
# one-sided on purpose: it must not reject what the reference's sanitisation would accept, and it accepts things RDKit rejects.
# This is the table's only copy: the kernel and the tests' restatement are handed it.
MAX_VALENCE = {5: 3, 6: 4, 7: 4, 8: 2, 9: 1, 14: 4, 15: 7, 16: 6, 17: 1, 35: 1, 53: 5}
assert list(MAX_VALENCE) == ATOM_TYPES
ELEMENT_SYMBOL = {5: 'B', 6: 'C', 7: 'N', 8: 'O', 9: 'F', 14: 'Si', 15: 'P', 16: 'S', 17: 'Cl', 35: 'Br', 53: 'I'}
MAX_ATOMS = hip.PG_MOL_MAX_ATOMS

_max_valence2 = {}               # device -> uint8 [11], twice MAX_VALENCE in class order


def _valence_table(device):
    t = _max_valence2.get(device)
    if t is None:
        t = _max_valence2[device] = torch.tensor([2 * MAX_VALENCE[z] for z in ATOM_TYPES], dtype=torch.uint8, device=device)
    return t


@dataclass
class Screen:
    """Device tensors of one `screen` call; F frames, B graphs, N atom rows, E directed bond rows (H = E / 2 pairs a < b)."""
    status: torch.Tensor         # int32 [F, B]   STATUS_* bits
    counts: torch.Tensor         # int32 [F, B, 4] kept atoms, bonds, components, atoms of the largest component
    valid: torch.Tensor          # bool  [F, B]   no bit of FAIL_MASK
    cls: torch.Tensor            # int8  [F, N]   atom class, -1 = dropped
    compact: torch.Tensor        # int16 [F, N]   index among the kept atoms of the graph, -1 = dropped
    valence2: torch.Tensor       # uint8 [F, N]   twice the valence (aromatic = 1.5), saturating at 255
    comp: torch.Tensor           # int16 [F, N]   smallest local atom index of the atom's component, -1 = dropped
    order: torch.Tensor          # int8  [F, H]   bond order of the pair rows (0 = none, 4 = aromatic); graph g starts at bond_off[g] / 2
    lig_off: torch.Tensor        # int32 [B + 1]
    bond_off: torch.Tensor       # int32 [B + 1]  (directed rows, both halves)
    num_atoms: list              # B ints


def _frames(results, frames):
    if frames == 'final':
        node, pos, edge = results['pred']
        return node, pos, edge, 1, (0, 0, 0)
    if frames == 'traj':
        node, pos, edge = results['traj']
        if node is None or pos is None or edge is None:
            raise ValueError("phoregen_amd.molecule.screen: frames='traj' needs a result sampled with return_traj=True")
        if not (node.dim() == pos.dim() == edge.dim() == 3 and node.size(0) == pos.size(0) == edge.size(0)):
            raise ValueError('phoregen_amd.molecule.screen: trajectory tensors must be [frames, rows, .] with one frame count')
        return node, pos, edge, node.size(0), (node.stride(0), edge.stride(0), pos.stride(0))
    raise ValueError(f"phoregen_amd.molecule.screen: frames must be 'final' or 'traj', not {frames!r}")


@torch.no_grad()
def screen(results, frames='final'):
    """Decode and screen every graph of a `sample` / `sample_batch` result on the device its tensors live on.
    frames='final': the final prediction (`results['pred']`, F = 1); 'traj': every frame of the saved trajectory.
    `results` is only read."""
    node, pos, edge, F, (node_fs, edge_fs, pos_fs) = _frames(results, frames)
    dev = node.device
    if dev.type != 'cuda':
        raise RuntimeError('phoregen_amd.molecule.screen: the screen is a HIP kernel and the result lives on %s; there is no CPU '
                           'fallback' % dev)
    for t, k, what in ((node, 12, 'atom scores'), (pos, 3, 'coordinates'), (edge, 6, 'bond scores')):
        row = t[0] if t.dim() == 3 and F > 0 else t
        if t.dtype != torch.float32 or t.device != dev or t.size(-1) != k or not (row.is_contiguous() or row.numel() == 0):
            raise ValueError(f'phoregen_amd.molecule.screen: {what} must be contiguous fp32 [.., {k}] on one device')
    N, E = node.size(-2), edge.size(-2)
    na = results['lig_info'][0].to(dev).long().reshape(-1)
    B = na.numel()
    with torch.cuda.device(dev):
        lib = hip.lib()
        lig_off = torch.zeros(B + 1, dtype=torch.long, device=dev)
        bond_off = torch.zeros(B + 1, dtype=torch.long, device=dev)
        lig_off[1:], bond_off[1:] = na.cumsum(0), (na * (na - 1)).cumsum(0)
        num_atoms = na.tolist()                                        # (the one host read of this call)
        if any(n < 0 for n in num_atoms) or sum(num_atoms) != N or pos.size(-2) != N:
            raise ValueError(f'phoregen_amd.molecule.screen: num_atoms sum to {sum(num_atoms)}, the result has {N} atom rows')
        if sum(n * (n - 1) for n in num_atoms) != E:
            raise ValueError(f'phoregen_amd.molecule.screen: {E} bond rows, num_atoms imply {sum(n * (n - 1) for n in num_atoms)} '
                             '(fully connected, both directions)')
        lig_off, bond_off = lig_off.int(), bond_off.int()
        H = E // 2
        out = dict(status=torch.empty(F, B, dtype=torch.int32, device=dev), counts=torch.empty(F, B, 4, dtype=torch.int32, device=dev),
                   cls=torch.empty(F, N, dtype=torch.int8, device=dev), compact=torch.empty(F, N, dtype=torch.int16, device=dev),
                   valence2=torch.empty(F, N, dtype=torch.uint8, device=dev), comp=torch.empty(F, N, dtype=torch.int16, device=dev),
                   order=torch.empty(F, H, dtype=torch.int8, device=dev))
        _launch(lib, node, node_fs, edge, edge_fs, pos, pos_fs, lig_off, bond_off, B, F, N, E, max(num_atoms, default=0), out)
    return Screen(valid=(out['status'] & FAIL_MASK) == 0, lig_off=lig_off, bond_off=bond_off, num_atoms=num_atoms, **out)


def _launch(lib, node, node_fs, edge, edge_fs, pos, pos_fs, lig_off, bond_off, B, F, N, E, max_n, out):
    """pg_mol_screen on the current stream.  A graph above MAX_ATOMS is the library's error (RuntimeError with its message): nothing
    is launched and `out` is not written."""
    hip.check(lib.pg_mol_screen(node.data_ptr(), node_fs, edge.data_ptr(), edge_fs, pos.data_ptr(), pos_fs, lig_off.data_ptr(),
                                bond_off.data_ptr(), B, F, N, E, max_n, _valence_table(node.device).data_ptr(),
                                out['status'].data_ptr(), out['counts'].data_ptr(), out['cls'].data_ptr(),
                                out['compact'].data_ptr(), out['valence2'].data_ptr(), out['comp'].data_ptr(),
                                out['order'].data_ptr(), hip.stream_ptr()), 'pg_mol_screen')


_PAIRS = {}


def _pairs(n):
    """The pairs a < b of n atoms in row-major order: the first half of a graph's bond rows (plan.make_edge_data)."""
    p = _PAIRS.get(n)
    if p is None:
        a, b = np.triu_indices(n, 1)
        p = _PAIRS[n] = (a.astype(np.int64), b.astype(np.int64))
    return p


@torch.no_grad()
def assemble(results):
    """The final prediction as one dict per graph with `decode_data`'s keys and meaning -- 'element' (atomic numbers), 'atom_pos'
    (kept atoms, the tensor's own fp32 values), 'bond_index' [2, n_b] (indices among the kept atoms) and 'bond_type' [n_b] for
    a < b only, in row order -- plus 'status', 'valid', 'n_components' and 'valence' (per kept atom, halves allowed).  The screen runs
    on the device; ONE device-to-host copy brings the compact arrays over, the split by offsets is on the host."""
    sc = screen(results, 'final')
    parts = [sc.status[0], sc.counts[0], results['pred'][1], sc.compact[0], sc.cls[0], sc.valence2[0], sc.order[0]]
    sizes = [p.numel() * p.element_size() for p in parts]
    blob = torch.cat([p.reshape(-1).view(torch.uint8) for p in parts]).cpu().numpy()
    cut = np.cumsum([0] + sizes)
    status, counts, pos, compact, cls, valence2, order = (
        blob[cut[i]:cut[i + 1]].view(dt) for i, dt in enumerate((np.int32, np.int32, np.float32, np.int16, np.int8, np.uint8, np.int8)))
    counts, pos = counts.reshape(-1, 4), pos.reshape(-1, 3)
    mols, n0, h0 = [], 0, 0
    for g, n in enumerate(sc.num_atoms):
        h = n * (n - 1) // 2
        keep = cls[n0:n0 + n] >= 0
        o = order[h0:h0 + h]
        nz = np.nonzero(o)[0]
        a, b = _pairs(n)
        cmp_g = compact[n0:n0 + n].astype(np.int64)
        mols.append({'element': [ATOM_TYPES[c] for c in cls[n0:n0 + n][keep].tolist()],
                     'atom_pos': torch.from_numpy(pos[n0:n0 + n][keep]),
                     'bond_index': torch.from_numpy(np.stack([cmp_g[a[nz]], cmp_g[b[nz]]])),
                     'bond_type': torch.from_numpy(o[nz].astype(np.int64)),
                     'status': int(status[g]), 'valid': (int(status[g]) & FAIL_MASK) == 0, 'n_components': int(counts[g, 2]),
                     'valence': valence2[n0:n0 + n][keep].astype(np.float64) / 2.0})
        n0, h0 = n0 + n, h0 + h
    return mols


# ---- V2000 mol blocks (CTfile format) ---------------------------------------------------------------------------------------
def mol_block(mol, name=''):
    """One V2000 mol block of an assembled molecule: three header lines (name, program line with the '3D' flag, empty comment),
    the counts line, one line per atom and per bond (type 4 = aromatic), 'M  END'."""
    elements, pos = mol['element'], np.asarray(mol['atom_pos'], dtype=np.float64).reshape(-1, 3)
    bi, bt = np.asarray(mol['bond_index']).reshape(2, -1), np.asarray(mol['bond_type']).reshape(-1)
    if len(elements) > 999 or bt.size > 999:
        raise ValueError(f'mol_block: {len(elements)} atoms / {bt.size} bonds do not fit the 3-digit counts of a V2000 block')
    if not np.isfinite(pos).all():
        raise ValueError('mol_block: non-finite coordinates')
    lines = [str(name).split('\n')[0], '  PhoreGen' + ' ' * 10 + '3D', '',
             '%3d%3d  0  0  0  0  0  0  0  0999 V2000' % (len(elements), bt.size)]
    for z, (x, y, zc) in zip(elements, pos.tolist()):
        lines.append('%10.4f%10.4f%10.4f %-3s 0  0  0  0  0  0  0  0  0  0  0  0' % (x, y, zc, ELEMENT_SYMBOL[int(z)]))
    for (a, b), t in zip(bi.T.tolist(), bt.tolist()):
        lines.append('%3d%3d%3d  0' % (a + 1, b + 1, t))
    lines.append('M  END')
    return '\n'.join(lines) + '\n'


def write_sdf(path, mols, names=None):
    """An SDF file: one mol block per molecule, each closed by a '$$$$' line."""
    names = names if names is not None else [''] * len(mols)
    if len(names) != len(mols):
        raise ValueError(f'write_sdf: {len(mols)} molecules, {len(names)} names')
    with open(path, 'w') as fh:
        for m, nm in zip(mols, names):
            fh.write(mol_block(m, nm))
            fh.write('$$$$\n')


# ---- the top-up loop of sample_all.py:79-84,172 ------------------------------------------------------------------------------
def sample_valid(model, data, num_samples, batch_size=30, max_failed_factor=3, device='cuda', **sample_kwargs):
    """Sample until `num_samples` molecules have passed the screen, giving up once more than `max_failed_factor * num_samples` have
    failed (checked before every draw, as the reference does).  Every draw asks for min(batch_size, what is still missing) graphs,
    so never more than `num_samples` are finished.  `sample_kwargs` (fragment=, pos_guidance_opt=, rng=, seed=, ...) go to
    `model.sample`; a fixed seed= repeats the same draw in every call of the same size, so leave it unset (a fresh key per call, drawn
    from torch's default generator) unless that is meant.  Returns {'finished': [...], 'failed': [...], 'n_calls': int} with `assemble`'s dicts."""
    finished, failed, n_calls = [], [], 0
    while len(finished) < num_samples:
        if len(failed) > max_failed_factor * num_samples:
            break
        n = min(batch_size, num_samples - len(finished))
        res = model.sample(data, n, device, return_traj=False, **sample_kwargs)
        n_calls += 1
        for m in assemble(res):
            (finished if m['valid'] else failed).append(m)
    return {'finished': finished, 'failed': failed, 'n_calls': n_calls}
