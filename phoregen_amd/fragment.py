"""Fragment-conditioned sampling (an extension of this project's; the reference has no such mode): host-side spec and layout.

A fragment is n_f atoms with fixed types (classes 0..10 of ATOM_TYPES), world coordinates (the frame of the sampler's output) and
bonds (i, j, c), c in 1..4; every unlisted pair of fragment atoms is class 0 (no bond).  In a graph that carries one, the fragment
is the graph's first n_f atoms; a bond row i->j is fixed iff both ends are fragment atoms.  The sampler replaces the fixed rows
RePaint-style after every step (csrc/posterior.hip, `FRAG` kernels; DESIGN.md "Fragment-conditioned sampling").
"""
from dataclasses import dataclass

import torch

from .plan import make_edge_data
from .utils.sample_utils import ATOM_TYPES

NUM_FRAGMENT_CLASSES = len(ATOM_TYPES)     # 11: class 11 (masked atom) cannot be fixed
BOND_CLASSES = (1, 2, 3, 4)                # class 0 = no bond (implicit), 5 = absorbing state (refused)
# Philox stream ids of the replacement draws (0 - 2 are the posteriors' node / bond / position noise)
STREAM_NODE, STREAM_EDGE, STREAM_POS = 3, 4, 5


def _int(v, what):
    if isinstance(v, bool) or not float(v).is_integer():
        raise ValueError(f'fragment: {what} must be an integer (got {v!r})')
    return int(v)


@dataclass(frozen=True)
class Fragment:
    types: torch.Tensor      # [n_f] int64 class indices 0..10
    pos: torch.Tensor        # [n_f, 3] float32 world coordinates
    bonds: torch.Tensor      # [n_b, 3] int64 rows (i, j, c), i < j

    @property
    def n_atoms(self):
        return int(self.types.numel())

    @property
    def elements(self):
        return [ATOM_TYPES[c] for c in self.types.tolist()]

    @classmethod
    def from_dict(cls, d):
        """{'element': atomic numbers from ATOM_TYPES | 'type': class indices 0..10, 'pos': [n_f, 3], 'bonds': [(i, j, c), ...]}."""
        if isinstance(d, Fragment):
            return d
        if not isinstance(d, dict):
            raise ValueError(f'fragment: expected a dict, got {type(d).__name__}')
        unknown = set(d) - {'element', 'type', 'pos', 'bonds'}
        if unknown:
            raise ValueError(f'fragment: unknown keys {sorted(unknown)}')
        if ('element' in d) == ('type' in d):
            raise ValueError("fragment: give exactly one of 'element' (atomic numbers) and 'type' (class indices)")
        raw = d['element'] if 'element' in d else d['type']
        raw = raw.tolist() if torch.is_tensor(raw) else list(raw)
        if not raw:
            raise ValueError('fragment: at least one atom is needed')
        if 'element' in d:
            types = []
            for z in raw:
                z = _int(z, 'an element')
                if z not in ATOM_TYPES:
                    raise ValueError(f'fragment: element {z} is not one of the model\'s atom types {ATOM_TYPES}')
                types.append(ATOM_TYPES.index(z))
        else:
            types = [_int(c, 'a type class') for c in raw]
            bad = [c for c in types if not 0 <= c < NUM_FRAGMENT_CLASSES]
            if bad:
                raise ValueError(f'fragment: type classes must be in 0..{NUM_FRAGMENT_CLASSES - 1} (class 11 = masked atom), got {bad}')
        n = len(types)
        if 'pos' not in d:
            raise ValueError("fragment: 'pos' is required")
        pos = torch.as_tensor(d['pos'], dtype=torch.float64)
        if pos.shape != (n, 3):
            raise ValueError(f'fragment: pos must have shape [{n}, 3], got {list(pos.shape)}')
        if not torch.isfinite(pos).all():
            raise ValueError('fragment: pos must be finite')
        bonds, seen = [], {}
        raw_b = d.get('bonds', [])
        raw_b = raw_b.tolist() if torch.is_tensor(raw_b) else list(raw_b)
        for b in raw_b:
            b = list(b)
            if len(b) != 3:
                raise ValueError(f'fragment: a bond is (i, j, class), got {b!r}')
            i, j, c = (_int(v, 'a bond field') for v in b)
            if not (0 <= i < n and 0 <= j < n):
                raise ValueError(f'fragment: bond ({i}, {j}) indexes outside the {n} fragment atoms')
            if i == j:
                raise ValueError(f'fragment: bond ({i}, {j}) joins an atom to itself')
            if c not in BOND_CLASSES:
                raise ValueError(f'fragment: bond class must be in 1..4, got {c} for ({i}, {j})')
            key = (min(i, j), max(i, j))
            if key in seen:
                kind = 'duplicate' if seen[key] == c else 'contradictory'
                raise ValueError(f'fragment: {kind} bond {key} (classes {seen[key]} and {c})')
            seen[key] = c
            bonds.append((key[0], key[1], c))
        return cls(torch.tensor(types, dtype=torch.long), pos.float().contiguous(),
                   torch.tensor(bonds, dtype=torch.long).reshape(-1, 3))

    def to_dict(self):
        return {'element': self.elements, 'pos': self.pos.tolist(), 'bonds': self.bonds.tolist()}

    def bond_matrix(self):
        """[n_f, n_f] class of every ordered pair (0 = no bond; symmetric)."""
        m = torch.zeros(self.n_atoms, self.n_atoms, dtype=torch.long)
        if self.bonds.numel():
            i, j, c = self.bonds.unbind(1)
            m[i, j] = c
            m[j, i] = c
        return m


def as_fragment(f):
    return None if f is None else Fragment.from_dict(f)


def fragment_atom_counts(num_atoms, fragment, explicit):
    """Atom counts of `sample(..., fragment=...)`: an explicit count below n_f is an error; a drawn count is raised to n_f + 1
    (at least one atom is generated)."""
    num_atoms = torch.as_tensor(num_atoms).long()
    if fragment is None:
        return num_atoms
    nf = fragment.n_atoms
    if explicit:
        if bool((num_atoms < nf).any()):
            raise ValueError(f'num_atoms {num_atoms.tolist()} has a count below the fragment\'s {nf} atoms')
        return num_atoms
    return num_atoms.clamp(min=nf + 1)


@dataclass
class FragmentLayout:
    node_cls: torch.Tensor     # [N] int32 fixed class, -1 = free
    edge_cls: torch.Tensor     # [E] int32 fixed bond class (0 = no bond), -1 = free
    x0f: torch.Tensor          # [N, 3] float32 fragment coordinates - the graph's centre (0 on free rows)
    pos: torch.Tensor          # [N, 3] float32 fragment world coordinates (0 on free rows)

    @property
    def node_fixed(self):
        return self.node_cls >= 0

    @property
    def edge_fixed(self):
        return self.edge_cls >= 0

    def to(self, device):
        return FragmentLayout(*(t.to(device) for t in (self.node_cls, self.edge_cls, self.x0f, self.pos)))


def fragment_layout(num_atoms, fragments, centers=None, edge_index=None):
    """Per-row tables of a batch: num_atoms [B], fragments = B entries (Fragment / dict / None), centers [B, 3] (the frame the
    sampler adds back; default 0), edge_index = make_edge_data(num_atoms)[0] (computed when not given).  Returns None when no
    graph carries a fragment."""
    num_atoms = torch.as_tensor(num_atoms).detach().cpu().long()
    B = int(num_atoms.numel())
    fragments = list(fragments)
    if len(fragments) != B:
        raise ValueError(f'fragments: expected {B} entries (one per graph, None allowed), got {len(fragments)}')
    frags = [as_fragment(f) for f in fragments]
    if all(f is None for f in frags):
        return None
    if edge_index is None:
        edge_index, _ = make_edge_data(num_atoms)
    edge_index = edge_index.detach().cpu().long()
    centers = torch.zeros(B, 3) if centers is None else torch.as_tensor(centers).detach().cpu().float().reshape(B, 3)
    N, E = int(num_atoms.sum()), int(edge_index.size(1))
    off = torch.zeros(B + 1, dtype=torch.long)
    off[1:] = num_atoms.cumsum(0)
    e_off = torch.zeros(B + 1, dtype=torch.long)
    e_off[1:] = (num_atoms * (num_atoms - 1)).cumsum(0)
    if int(e_off[-1]) != E:
        raise ValueError('fragment_layout: edge_index is not the fully connected edge list of num_atoms')
    node_cls = torch.full((N,), -1, dtype=torch.int32)
    edge_cls = torch.full((E,), -1, dtype=torch.int32)
    x0f, pos = torch.zeros(N, 3), torch.zeros(N, 3)
    for g, f in enumerate(frags):
        if f is None:
            continue
        nf, n0 = f.n_atoms, int(off[g])
        if nf > int(num_atoms[g]):
            raise ValueError(f'graph {g} has {int(num_atoms[g])} atoms, fewer than its fragment\'s {nf}')
        node_cls[n0:n0 + nf] = f.types.to(torch.int32)
        pos[n0:n0 + nf] = f.pos
        x0f[n0:n0 + nf] = f.pos - centers[g]
        e0, e1 = int(e_off[g]), int(e_off[g + 1])
        src, dst = edge_index[0, e0:e1] - n0, edge_index[1, e0:e1] - n0
        fixed = (src < nf) & (dst < nf)
        m = f.bond_matrix()
        edge_cls[e0:e1][fixed] = m[src[fixed], dst[fixed]].to(torch.int32)
    return FragmentLayout(node_cls, edge_cls, x0f, pos)


def load_fragment_json(path):
    import json
    with open(path) as fh:
        return Fragment.from_dict(json.load(fh))


__all__ = ['Fragment', 'FragmentLayout', 'as_fragment', 'fragment_atom_counts', 'fragment_layout', 'load_fragment_json',
           'STREAM_NODE', 'STREAM_EDGE', 'STREAM_POS', 'NUM_FRAGMENT_CLASSES']
