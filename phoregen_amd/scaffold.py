"""Murcko scaffolds, frameworks and scaffold grouping of decoded molecules on the device (csrc/mol_scaffold.hip; DESIGN.md 2.9
"Scaffolds").

`scaffolds` writes the scaffold of every (frame, graph) of a `Screen` as a `Screen` of its own, with the same layout: atoms outside
the scaffold are dropped (class -1) and bonds outside it are 0.  Everything that takes a screen then works on scaffolds unchanged:
`scaffold_keys` is `molecule_keys` of the scaffold screen, scaffold similarity is `fingerprints` of it, scaffold SMILES is `kekulize` +
`smiles` with `screen=` the scaffold screen, scaffold molecules are `assemble(results, screen=)`.

The scaffold: the core is what is left after every atom with at most one remaining neighbour has been removed, again and again (empty
for a molecule without a ring); a bond of the core is a ring bond if a ring passes through it (the search of `molecule.rings`), else
a linker bond; an atom of the core with a ring bond is a ring atom, any other a linker atom.  `exocyclic=True` (the default, the
RDKit-style Murcko convention) also keeps every atom outside the core that has a bond of order exactly 2 to an atom of the core -- ring
and linker `=O` -- and nothing else of it; `exocyclic=False` is the plain Bemis-Murcko framework.  `generic=True` then gives every
scaffold atom carbon's class and every scaffold bond order 1.  With `generic=True, exocyclic=True` a second pass over the scaffold
drops the former exocyclic atoms (their bonds are single by then); every other combination reproduces itself.  Exact integer work,
independent of the numbering of the atoms; graphs that failed the source screen are processed like any other.  Not checked against
RDKit.

`batch_of` turns assembled molecule dicts back into a sampler-shaped result, so that finished molecules collected over many draws (or
read back later) reach any device-side analysis; `scaffold_groups` and `pick_per_scaffold` answer which molecules share a scaffold
and pick at most k of each."""
from dataclasses import dataclass

import numpy as np
import torch

from . import hip
from .molecule import FAIL_MASK, Screen, _check_arrays, _need_cuda, duplicate_groups, molecule_keys, same_molecule
from .plan import make_edge_data
from .utils.sample_utils import ATOM_TYPES

PART_NONE, PART_SIDE_CHAIN, PART_LINKER, PART_RING, PART_EXOCYCLIC = range(5)      # values of `Scaffolds.part` (PG_SCAF_PART_*)
SCAFFOLD_COUNTS = ('scaffold_atoms', 'scaffold_bonds', 'ring_atoms', 'linker_atoms', 'exocyclic_atoms', 'side_chain_atoms',
                   'ring_systems', 'linker_bonds')
_M64 = (1 << 64) - 1


@dataclass(frozen=True)
class ScaffoldOptions:
    """exocyclic: also keep atoms double-bonded to the core (RDKit-style Murcko scaffold; False: plain Bemis-Murcko framework).
    generic: carbon's class for every scaffold atom and order 1 for every scaffold bond, after the selection."""
    exocyclic: bool = True
    generic: bool = False

    def __post_init__(self):
        for name in ('exocyclic', 'generic'):
            if not isinstance(getattr(self, name), (bool, np.bool_)):
                raise ValueError(f'phoregen_amd.scaffold.ScaffoldOptions: {name} must be a bool, not {getattr(self, name)!r}')

    @property
    def flags(self):
        return (hip.PG_SCAF_EXOCYCLIC if self.exocyclic else 0) | (hip.PG_SCAF_GENERIC if self.generic else 0)


@dataclass
class Scaffolds:
    """Device tensors of one `scaffolds` call; F frames, B graphs, N atom rows."""
    part: torch.Tensor           # uint8 [F, N]    PART_*: 0 not kept, 1 side chain, 2 linker, 3 ring, 4 exocyclic
    counts: torch.Tensor         # int32 [F, B, 8] SCAFFOLD_COUNTS
    screen: Screen               # the scaffold as a screen: same layout and offsets as `source`; status has NO_ATOMS / DISCONNECTED only
    options: ScaffoldOptions
    source: Screen               # the screen it was computed from


@torch.no_grad()
def scaffolds(sc, options=ScaffoldOptions()):
    """The scaffold of every (frame, graph) of a `Screen`, on its device, in one launch (pg_mol_scaffold).  `Scaffolds.screen` has the
    source's layout: `cls` the class (or carbon's) of a scaffold atom, else -1; `compact` the index among the graph's scaffold atoms;
    `order` the order (or 1) of a bond between two scaffold atoms, else 0; `valence2`, `comp` and `counts` computed on the scaffold;
    `status` carries only STATUS_NO_ATOMS (no scaffold atom: every acyclic molecule) and STATUS_DISCONNECTED -- no valence check is
    made on a scaffold, so `valid` says: one non-empty connected scaffold.  No host read."""
    if not isinstance(sc, Screen):
        raise ValueError(f'phoregen_amd.scaffold.scaffolds: needs a Screen (molecule.screen), not {type(sc).__name__}')
    if not isinstance(options, ScaffoldOptions):
        raise ValueError(f'phoregen_amd.scaffold.scaffolds: options must be a ScaffoldOptions, not {options!r}')
    dev = sc.cls.device
    _need_cuda('scaffolds', 'the scaffold', dev, 'screen')
    F, B = sc.status.shape
    N, H = sc.cls.size(1), sc.order.size(1)
    with torch.cuda.device(dev):
        lib = hip.lib()
        part = torch.empty(F, N, dtype=torch.uint8, device=dev)
        counts = torch.empty(F, B, len(SCAFFOLD_COUNTS), dtype=torch.int32, device=dev)
        out = dict(status=torch.empty(F, B, dtype=torch.int32, device=dev), counts=torch.empty(F, B, 4, dtype=torch.int32, device=dev),
                   cls=torch.empty(F, N, dtype=torch.int8, device=dev), compact=torch.empty(F, N, dtype=torch.int16, device=dev),
                   valence2=torch.empty(F, N, dtype=torch.uint8, device=dev), comp=torch.empty(F, N, dtype=torch.int16, device=dev),
                   order=torch.empty(F, H, dtype=torch.int8, device=dev))
        _launch_scaffold(lib, sc.cls, sc.order, sc.lig_off, sc.bond_off, B, F, max(sc.num_atoms, default=0), options.flags, part, counts, out)
    scaffold = Screen(valid=(out['status'] & FAIL_MASK) == 0, lig_off=sc.lig_off, bond_off=sc.bond_off, num_atoms=list(sc.num_atoms),
                      bonds=sc.bonds, agree=None, **out)
    return Scaffolds(part=part, counts=counts, screen=scaffold, options=options, source=sc)


def _launch_scaffold(lib, cls, order, lig_off, bond_off, B, F, max_n, flags, part, counts, out):
    """pg_mol_scaffold on the current stream.  A graph above MAX_ATOMS is the library's error: nothing is launched and the outputs
    are not written."""
    _check_arrays('scaffolds', cls.device, [(cls, torch.int8), (order, torch.int8), (lig_off, torch.int32), (bond_off, torch.int32),
                                            (part, torch.uint8), (counts, torch.int32), (out['status'], torch.int32),
                                            (out['counts'], torch.int32), (out['cls'], torch.int8), (out['compact'], torch.int16),
                                            (out['valence2'], torch.uint8), (out['comp'], torch.int16), (out['order'], torch.int8)])
    if (lig_off.numel() != B + 1 or bond_off.numel() != B + 1 or cls.numel() != F * cls.size(-1) or order.numel() != F * order.size(-1)
            or any(out[k].shape != cls.shape for k in ('cls', 'compact', 'valence2', 'comp')) or part.shape != cls.shape
            or out['order'].shape != order.shape or out['status'].numel() != F * B or out['counts'].numel() != 4 * F * B
            or counts.numel() != len(SCAFFOLD_COUNTS) * F * B):
        raise ValueError(f'phoregen_amd.scaffold.scaffolds: sizes of the offsets, screen arrays and outputs do not fit {F} frames x {B} '
                         f'graphs, {cls.size(-1)} atom rows, {order.size(-1)} pair rows')
    hip.check(lib.pg_mol_scaffold(cls.data_ptr(), order.data_ptr(), lig_off.data_ptr(), bond_off.data_ptr(), B, F, cls.size(-1),
                                  2 * order.size(-1), max_n, flags, part.data_ptr(), counts.data_ptr(), out['status'].data_ptr(),
                                  out['counts'].data_ptr(), out['cls'].data_ptr(), out['compact'].data_ptr(), out['valence2'].data_ptr(),
                                  out['comp'].data_ptr(), out['order'].data_ptr(), hip.stream_ptr()), 'pg_mol_scaffold')


def scaffold_keys(sf):
    """Identity keys of the scaffolds: `molecule_keys(sf.screen)`.  Every molecule without a ring has the empty scaffold and so the
    key KEY_EMPTY: acyclic molecules all fall into one group.  With `generic=True` this is the framework key.  Equal keys are
    necessary, not sufficient, for equal scaffolds (`scaffold_groups(keys, mols)` confirms)."""
    if not isinstance(sf, Scaffolds):
        raise ValueError(f'phoregen_amd.scaffold.scaffold_keys: needs a Scaffolds, not {type(sf).__name__}')
    return molecule_keys(sf.screen)


def batch_of(mols, device):
    """Assembled molecule dicts ('element' atomic numbers, 'atom_pos' [n, 3], 'bond_index' [2, n_b] among the molecule's atoms,
    'bond_type' [n_b] in 1..4) as a sampler-shaped result on `device`: 'pred' = [atom scores [N, 12], coordinates [N, 3], bond scores
    [E, 6]] with one-hot scores, the bond's class in both halves of the edge rows and class 0 for every other pair, 'traj' = [None] * 3,
    'lig_info' = [num_atoms, batch, edge_index, edge_batch].  `molecule.screen(batch_of(mols, device))` reproduces their atoms and
    bonds, in their order.  An element outside ATOM_TYPES, a bond type outside 1..4, or a bond that is a loop, a repeat or out of
    range raises ValueError."""
    sizes, node_cls, poss, edge_cls = [], [], [], []
    for g, m in enumerate(mols):
        el = [int(z) for z in m['element']]
        n = len(el)
        for z in el:
            if z not in ATOM_TYPES:
                raise ValueError(f'phoregen_amd.scaffold.batch_of: molecule {g} has element {z}, outside ATOM_TYPES {tuple(ATOM_TYPES)}')
        pos = torch.as_tensor(m['atom_pos'], dtype=torch.float32).reshape(-1, 3)
        if pos.size(0) != n:
            raise ValueError(f'phoregen_amd.scaffold.batch_of: molecule {g} has {n} elements and {pos.size(0)} coordinates')
        bi = np.asarray(torch.as_tensor(m['bond_index']).cpu(), dtype=np.int64).reshape(2, -1)
        bt = np.asarray(torch.as_tensor(m['bond_type']).cpu(), dtype=np.int64).reshape(-1)
        if bi.shape[1] != bt.size:
            raise ValueError(f'phoregen_amd.scaffold.batch_of: molecule {g} has {bi.shape[1]} bonds and {bt.size} bond types')
        if bt.size and (bt.min() < 1 or bt.max() > 4):
            raise ValueError(f'phoregen_amd.scaffold.batch_of: molecule {g} has a bond type outside 1..4 (4 = aromatic)')
        lo, hi = np.minimum(bi[0], bi[1]), np.maximum(bi[0], bi[1])
        if bt.size and (lo.min() < 0 or hi.max() >= n or (lo == hi).any()):
            raise ValueError(f'phoregen_amd.scaffold.batch_of: molecule {g} has a bond outside its {n} atoms or from an atom to itself')
        h = n * (n - 1) // 2
        rows = lo * n - lo * (lo + 1) // 2 + (hi - lo - 1)
        if np.unique(rows).size != rows.size:
            raise ValueError(f'phoregen_amd.scaffold.batch_of: molecule {g} lists a bond twice')
        half = np.zeros(h, dtype=np.int64)
        half[rows] = bt
        sizes.append(n)
        node_cls.append(np.array([ATOM_TYPES.index(z) for z in el], dtype=np.int64))
        poss.append(pos.cpu())
        edge_cls.append(np.concatenate([half, half]))
    na = torch.tensor(sizes, dtype=torch.long)
    N = int(na.sum())
    ncls = torch.from_numpy(np.concatenate(node_cls)) if node_cls else torch.zeros(0, dtype=torch.long)
    ecls = torch.from_numpy(np.concatenate(edge_cls)) if edge_cls else torch.zeros(0, dtype=torch.long)
    node = torch.zeros(N, 12)
    node[torch.arange(N), ncls] = 1.0
    edge = torch.zeros(ecls.numel(), 6)
    edge[torch.arange(ecls.numel()), ecls] = 1.0
    pos = torch.cat(poss) if poss else torch.zeros(0, 3)
    ei, eb = make_edge_data(na)
    return {'pred': [node.to(device), pos.to(device), edge.to(device)], 'traj': [None, None, None],
            'lig_info': [na.to(device), torch.repeat_interleave(torch.arange(len(sizes)), na).to(device), ei.to(device), eb.to(device)]}


def scaffold_groups(keys, mols=None):
    """Which rows share a scaffold.  keys: int64 [n] (`scaffold_keys(sf).key[f]`).  Returns (group, sizes): group[i] the index of the
    first row with the same scaffold as row i (so group[i] <= i, and group[i] == i for the first of a group), sizes[i] the size of
    row i's group; both int64 [n] on the keys' device.
    mols=None: rows are grouped by key alone -- equal keys are NECESSARY, not sufficient, for equal scaffolds.
    mols=the scaffold molecules (`assemble(results, screen=sf.screen)`, one per row): equal keys are confirmed with `same_molecule`
    inside each key's group, as `unique_molecules` does, so the answer is exact; this is a host loop."""
    if not torch.is_tensor(keys) or keys.dim() != 1 or keys.dtype != torch.int64:
        raise ValueError('phoregen_amd.scaffold.scaffold_groups: keys must be an int64 tensor [n], not '
                         f'{tuple(keys.shape) if torch.is_tensor(keys) else type(keys).__name__}'
                         f'{" of " + str(keys.dtype) if torch.is_tensor(keys) else ""}')
    n, dev = keys.numel(), keys.device
    if mols is None:
        first, _, k = duplicate_groups(keys)                           # (first occurrence of every distinct key, the key's index per row)
        group = first[k]
    else:
        if len(mols) != n:
            raise ValueError(f'phoregen_amd.scaffold.scaffold_groups: {n} keys and {len(mols)} molecules')
        by_key, first = {}, []
        for i, (k, m) in enumerate(zip(keys.tolist(), mols)):
            reps = by_key.setdefault(k & _M64, [])
            hit = next((r for r in reps if same_molecule(mols[r], m)), None)
            if hit is None:
                hit = i
                reps.append(i)
            first.append(hit)
        group = torch.tensor(first, dtype=torch.long, device=dev)
    sizes = torch.bincount(group, minlength=n)[group] if n else torch.zeros(0, dtype=torch.long, device=dev)
    return group, sizes


def pick_per_scaffold(group, k):
    """The indices of the first k rows of every group of `scaffold_groups`, ascending: int64 [m] on the group's device."""
    if not torch.is_tensor(group) or group.dim() != 1 or group.dtype != torch.int64:
        raise ValueError('phoregen_amd.scaffold.pick_per_scaffold: group must be the int64 tensor [n] of scaffold_groups')
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 0:
        raise ValueError(f'phoregen_amd.scaffold.pick_per_scaffold: k must be an integer >= 0, not {k!r}')
    n = group.numel()
    if n == 0:
        return torch.zeros(0, dtype=torch.long, device=group.device)
    # rank of a row inside its group, in row order: a stable sort by group keeps the rows of a group ascending
    srt, perm = torch.sort(group, stable=True)
    new = torch.ones(n, dtype=torch.bool, device=group.device)
    new[1:] = srt[1:] != srt[:-1]
    starts = new.nonzero().reshape(-1)
    rank = torch.arange(n, device=group.device) - starts[new.cumsum(0) - 1]
    return perm[rank < int(k)].sort().values
