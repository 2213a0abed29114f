"""Substructure search on the device (csrc/mol_sub.hip, csrc/sub_core.h; DESIGN.md 2.9 "Substructure"): does this molecule contain that
group, how often, and where.

A `Pattern` is a small connected graph of query atoms and query bonds with constraints -- an atom's element set, heavy-atom degree,
hydrogens, charge, ring membership and aromaticity, a bond's order set and ring flag -- written as a dict (`Pattern.from_dict`,
`load_patterns_json`), taken from a `Fragment` (`Pattern.from_fragment`) or cut out of an assembled molecule (`Pattern.from_molecule`).
`substructure` counts, for every decoded (frame, graph) and every pattern in one launch, the embeddings (injective maps of the query
atoms onto kept atoms that meet every constraint; further bonds between the images are allowed: a monomorphism, the SMARTS convention),
the distinct images of query atom 0 (`anchors`: with the pattern written around its central atom, the number of such groups), the atoms
that lie in an embedding and the lexicographically first embedding.  `find_matches` is the exact pure-Python enumerator over one of
`assemble`'s dicts, the counterpart of `same_molecule`.  `molecule.assemble(substructure=)`, `molecule.sample_valid(substructure=)` and
`molecule.write_sdf` carry the answers.

Necessary, not sufficient, in the project's usual sense: there is no SMARTS parser, there are no recursive or negated environments and
no stereo constraints; there is no count of unique atom sets (`embeddings / automorphisms` is not in general that number: use `anchors`
or `atom_mask`); aromatic is the model's bond class 4, not a perception; hydrogens and charges are `kekulize`'s.  Not checked against
RDKit."""
import json
from collections import deque
from dataclasses import dataclass, field

import numpy as np
import torch

from . import hip
from . import molecule as M
from .utils.sample_utils import ATOM_TYPES

MAX_ATOMS = hip.PG_SUB_MAX_ATOMS             # query atoms of a pattern (PG_SUB_MAX_ATOMS)
MAX_PATTERNS = hip.PG_SUB_MAX_PATTERNS       # rows of a table
MAX_STEPS = hip.PG_SUB_MAX_STEPS             # the largest work bound
DEFAULT_STEPS = 65536
PATTERN_BYTES = hip.PG_SUB_PATTERN_BYTES
N_CLASSES = len(ATOM_TYPES)

SUB_MATCHED = 1                  # informational: at least one embedding
SUB_NO_KEKULE = 2                # the pattern constrains hydrogens or charge and the graph has no Kekulé structure: no embedding
SUB_TRUNCATED = 4                # a root's search was abandoned at max_steps: counts are lower bounds
SUB_OUT_OF_BOUNDS = 8            # anchors outside the pattern's [min, max], or the pattern is bounded and truncated
SUB_NAMES = {SUB_MATCHED: 'MATCHED', SUB_NO_KEKULE: 'NO_KEKULE', SUB_TRUNCATED: 'TRUNCATED', SUB_OUT_OF_BOUNDS: 'OUT_OF_BOUNDS'}

_SYMBOL_CLASS = {M.ELEMENT_SYMBOL[z]: c for c, z in enumerate(ATOM_TYPES)}
_FLAG = {None: hip.PG_SUB_ANY, True: hip.PG_SUB_YES, False: hip.PG_SUB_NO}
_FLAG_BACK = {v: k for k, v in _FLAG.items()}
_ANY_RANGE = (0, 255)


def _err(what):
    return ValueError(f'pattern: {what}')


def _int(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise _err(f'{what} must be an integer (got {v!r})')
    return int(v)


def _tri(v, what):
    if v is None or isinstance(v, (bool, np.bool_)):
        return None if v is None else bool(v)
    raise _err(f'{what} must be true, false or null (got {v!r})')


def _range(v, what):
    if v is None:
        return _ANY_RANGE
    if isinstance(v, (int, np.integer)) and not isinstance(v, bool):
        v = (v, v)
    if not isinstance(v, (list, tuple)) or len(v) != 2:
        raise _err(f'{what} must be an integer or [lo, hi] (got {v!r})')
    lo, hi = _int(v[0], what), _int(v[1], what)
    if not 0 <= lo <= hi <= 255:
        raise _err(f'{what} must satisfy 0 <= lo <= hi <= 255 (got {[lo, hi]})')
    return lo, hi


@dataclass(frozen=True)
class QueryAtom:
    """Constraints on the image of one query atom; None / (0, 255) = any."""
    elements: tuple = tuple(range(N_CLASSES))    # atom classes 0..10, sorted
    degree: tuple = _ANY_RANGE                   # (lo, hi) on the kept bonds of the atom
    hcount: tuple = _ANY_RANGE                   # (lo, hi) on `Kekule.hcount`
    charge: object = None                        # None, 0 or 1
    ring: object = None                          # None, True (atom_ring > 0), False
    aromatic: object = None                      # None, True (has a bond of order 4), False

    @property
    def uses_kekule(self):
        return self.hcount != _ANY_RANGE or self.charge is not None


@dataclass(frozen=True)
class QueryBond:
    """A query bond between query atoms a < b: the accepted orders (4 = aromatic) and the ring flag (True: ring_size > 0)."""
    a: int
    b: int
    orders: tuple = (1, 2, 3, 4)
    ring: object = None


def _elements(v, what):
    if v is None:
        return tuple(range(N_CLASSES))
    if not isinstance(v, (list, tuple, set, frozenset)) or len(v) == 0:
        raise _err(f'{what} must be a non-empty list of element symbols or atomic numbers (got {v!r})')
    out = set()
    for e in v:
        if isinstance(e, str):
            if e not in _SYMBOL_CLASS:
                raise _err(f'{what}: {e!r} is not one of the model\'s elements {sorted(_SYMBOL_CLASS)}')
            out.add(_SYMBOL_CLASS[e])
        else:
            z = _int(e, what)
            if z not in ATOM_TYPES:
                raise _err(f'{what}: {z} is not one of the model\'s atom types {ATOM_TYPES}')
            out.add(ATOM_TYPES.index(z))
    return tuple(sorted(out))


def _atom_from(d, i):
    what = f'atoms[{i}]'
    if not isinstance(d, dict):
        raise _err(f'{what} must be a dict (got {type(d).__name__})')
    unknown = set(d) - {'elements', 'degree', 'hcount', 'charge', 'ring', 'aromatic'}
    if unknown:
        raise _err(f'{what}: unknown keys {sorted(unknown)}')
    charge = d.get('charge')
    if charge is not None and (isinstance(charge, bool) or charge not in (0, 1)):
        raise _err(f'{what}.charge must be 0, 1 or null (got {charge!r})')
    return QueryAtom(_elements(d.get('elements'), what + '.elements'), _range(d.get('degree'), what + '.degree'),
                     _range(d.get('hcount'), what + '.hcount'), None if charge is None else int(charge),
                     _tri(d.get('ring'), what + '.ring'), _tri(d.get('aromatic'), what + '.aromatic'))


def _bond_from(d, i, k):
    what = f'bonds[{i}]'
    if not isinstance(d, dict):
        raise _err(f'{what} must be a dict (got {type(d).__name__})')
    unknown = set(d) - {'a', 'b', 'orders', 'ring'}
    if unknown:
        raise _err(f'{what}: unknown keys {sorted(unknown)}')
    if 'a' not in d or 'b' not in d:
        raise _err(f"{what} needs 'a' and 'b'")
    a, b = _int(d['a'], what + '.a'), _int(d['b'], what + '.b')
    if not (0 <= a < k and 0 <= b < k):
        raise _err(f'{what} ({a}, {b}) indexes outside the {k} query atoms')
    if a == b:
        raise _err(f'{what} ({a}, {b}) joins an atom to itself')
    orders = d.get('orders')
    if orders is None:
        orders = (1, 2, 3, 4)
    if not isinstance(orders, (list, tuple, set, frozenset)) or len(orders) == 0:
        raise _err(f'{what}.orders must be a non-empty subset of [1, 2, 3, 4] (got {orders!r})')
    orders = tuple(sorted({_int(o, what + '.orders') for o in orders}))
    if orders[0] < 1 or orders[-1] > 4:
        raise _err(f'{what}.orders must be a non-empty subset of [1, 2, 3, 4] (got {list(orders)})')
    return QueryBond(min(a, b), max(a, b), orders, _tri(d.get('ring'), what + '.ring'))


def _match_order(k, bonds):
    """Breadth-first from query atom 0, neighbours in ascending index; shorter than k for a disconnected pattern."""
    nbr = [[] for _ in range(k)]
    for b in bonds:
        nbr[b.a].append(b.b)
        nbr[b.b].append(b.a)
    order, seen, todo = [0], {0}, deque([0])
    while todo:
        u = todo.popleft()
        for v in sorted(nbr[u]):
            if v not in seen:
                seen.add(v)
                order.append(v)
                todo.append(v)
    return tuple(order)


@dataclass(frozen=True)
class Pattern:
    """A substructure pattern: `atoms` (QueryAtom), `bonds` (QueryBond, every pair at most once), and the bounds `min` / `max` on
    `anchors` that `Substructure.ok`, `sample_valid(substructure=)` and the command line filter on (0 / None: informational only).
    Query atom 0 is the anchor; `match_order` is the breadth-first order from it (neighbours ascending) in which embeddings are
    enumerated and compared."""
    name: str
    atoms: tuple
    bonds: tuple = ()
    min: int = 0
    max: object = None
    match_order: tuple = field(default=None)

    def __post_init__(self):
        if not isinstance(self.name, str) or not self.name or any(c.isspace() for c in self.name):
            raise _err(f'name must be a non-empty string without white space (got {self.name!r})')
        atoms, bonds = tuple(self.atoms), tuple(self.bonds)
        k = len(atoms)
        if not 1 <= k <= MAX_ATOMS:
            raise _err(f'atoms: {k} query atoms, a pattern has 1 .. {MAX_ATOMS}')
        if not all(isinstance(a, QueryAtom) for a in atoms) or not all(isinstance(b, QueryBond) for b in bonds):
            raise _err('atoms must be QueryAtom and bonds QueryBond objects (use Pattern.from_dict for dicts)')
        for i, a in enumerate(atoms):
            if not a.elements or any(not 0 <= c < N_CLASSES for c in a.elements):
                raise _err(f'atoms[{i}].elements must be a non-empty set of classes 0..{N_CLASSES - 1}')
        seen = set()
        for i, b in enumerate(bonds):
            if not (0 <= b.a < b.b < k):
                raise _err(f'bonds[{i}] ({b.a}, {b.b}) must join two of the {k} query atoms, a < b')
            if not b.orders or any(o not in (1, 2, 3, 4) for o in b.orders):
                raise _err(f'bonds[{i}].orders must be a non-empty subset of [1, 2, 3, 4]')
            if (b.a, b.b) in seen:
                raise _err(f'bonds: duplicate bond ({b.a}, {b.b})')
            seen.add((b.a, b.b))
        bonds = tuple(sorted(bonds, key=lambda b: (b.a, b.b)))
        lo = _int(self.min, 'min')
        hi = None if self.max is None else _int(self.max, 'max')
        if lo < 0 or (hi is not None and hi < lo) or lo > 0x7fffffff or (hi or 0) > 0x7fffffff:
            raise _err(f'min / max must satisfy 0 <= min <= max <= 2**31 - 1 (got {lo}, {hi})')
        order = _match_order(k, bonds)
        if len(order) != k:
            raise _err(f'bonds: the pattern is disconnected: query atoms {sorted(set(range(k)) - set(order))} cannot be reached from atom 0')
        if self.match_order is not None and tuple(self.match_order) != order:
            raise _err(f'match_order is computed (breadth-first from atom 0: {list(order)}), not chosen')
        for name, v in (('atoms', atoms), ('bonds', bonds), ('min', lo), ('max', hi), ('match_order', order)):
            object.__setattr__(self, name, v)

    @property
    def k(self):
        return len(self.atoms)

    @property
    def bounded(self):
        return self.min > 0 or self.max is not None

    @property
    def uses_kekule(self):
        return any(a.uses_kekule for a in self.atoms)

    @property
    def uses_rings(self):
        return any(a.ring is not None for a in self.atoms) or any(b.ring is not None for b in self.bonds)

    @classmethod
    def from_dict(cls, d):
        """{'name', 'atoms': [{'elements': ['C', 7, ..], 'degree': n or [lo, hi], 'hcount': n or [lo, hi], 'charge': 0 / 1, 'ring':
        bool, 'aromatic': bool}], 'bonds': [{'a', 'b', 'orders': [1..4], 'ring': bool}], 'min', 'max'}; every constraint is optional
        (absent or null = any).  Unknown keys, empty sets, a disconnected pattern and more than MAX_ATOMS atoms are errors."""
        if not isinstance(d, dict):
            raise _err(f'expected a dict, got {type(d).__name__}')
        unknown = set(d) - {'name', 'atoms', 'bonds', 'min', 'max'}
        if unknown:
            raise _err(f'unknown keys {sorted(unknown)}')
        if 'name' not in d or 'atoms' not in d:
            raise _err("'name' and 'atoms' are required")
        atoms = d['atoms']
        if not isinstance(atoms, (list, tuple)) or not 1 <= len(atoms) <= MAX_ATOMS:
            raise _err(f'atoms: a pattern has 1 .. {MAX_ATOMS} query atoms (got {len(atoms) if isinstance(atoms, (list, tuple)) else atoms!r})')
        bonds = d.get('bonds') or ()
        if not isinstance(bonds, (list, tuple)):
            raise _err(f'bonds must be a list (got {bonds!r})')
        return cls(d['name'], tuple(_atom_from(a, i) for i, a in enumerate(atoms)),
                   tuple(_bond_from(b, i, len(atoms)) for i, b in enumerate(bonds)), d.get('min') or 0, d.get('max'))

    def to_dict(self):
        atoms = []
        for a in self.atoms:
            e = {}
            if a.elements != tuple(range(N_CLASSES)):
                e['elements'] = [M.ELEMENT_SYMBOL[ATOM_TYPES[c]] for c in a.elements]
            if a.degree != _ANY_RANGE:
                e['degree'] = list(a.degree)
            if a.hcount != _ANY_RANGE:
                e['hcount'] = list(a.hcount)
            for key in ('charge', 'ring', 'aromatic'):
                if getattr(a, key) is not None:
                    e[key] = getattr(a, key)
            atoms.append(e)
        bonds = []
        for b in self.bonds:
            e = {'a': b.a, 'b': b.b}
            if b.orders != (1, 2, 3, 4):
                e['orders'] = list(b.orders)
            if b.ring is not None:
                e['ring'] = b.ring
            bonds.append(e)
        return {'name': self.name, 'atoms': atoms, 'bonds': bonds, 'min': self.min, 'max': self.max}

    @classmethod
    def from_fragment(cls, fragment, name='fragment', min=0, max=None):
        """The pattern of a `Fragment`: its atoms with their exact elements, its listed bonds with their exact classes.  Pairs of
        fragment atoms the fragment lists no bond for are NOT enforced to be unbonded (an embedding is a monomorphism), and a
        fragment whose listed bonds do not connect it is an error here.  Fragment atom i is query atom i, so atom 0 is the anchor."""
        from .fragment import as_fragment
        f = as_fragment(fragment)
        if f is None:
            raise _err('from_fragment needs a fragment')
        bonds = sorted((QueryBond(int(i), int(j), (int(c),)) for i, j, c in f.bonds.tolist()), key=lambda b: (b.a, b.b))
        return cls(name, tuple(QueryAtom((int(c),)) for c in f.types.tolist()), tuple(bonds), min, max)

    @classmethod
    def from_molecule(cls, mol, atoms=None, name='molecule', min=0, max=None):
        """The pattern of the atoms `atoms` (indices into the dict's atoms, default all; the first is the anchor) of one of
        `assemble`'s dicts: exact elements, and the bonds among them with their exact orders.  Nothing else is constrained."""
        n = len(mol['element'])
        pick = list(range(n)) if atoms is None else [_int(a, 'atoms') for a in atoms]
        if len(set(pick)) != len(pick) or any(not 0 <= a < n for a in pick):
            raise _err(f'atoms {pick} must be distinct indices into the molecule\'s {n} atoms')
        at = {a: i for i, a in enumerate(pick)}
        bi, bt = np.asarray(mol['bond_index']).reshape(2, -1), np.asarray(mol['bond_type']).reshape(-1)
        bonds = [QueryBond(*sorted((at[int(a)], at[int(b)])), (int(t),)) for a, b, t in zip(bi[0], bi[1], bt) if int(a) in at and int(b) in at]
        return cls(name, tuple(QueryAtom((ATOM_TYPES.index(int(mol['element'][a])),)) for a in pick), tuple(bonds), min, max)


def load_patterns_json(path):
    """A JSON file with a list of pattern dicts (or {'patterns': [...]}) -> [Pattern]."""
    with open(path) as fh:
        d = json.load(fh)
    if isinstance(d, dict) and set(d) == {'patterns'}:
        d = d['patterns']
    if not isinstance(d, list) or not d:
        raise _err(f'{path}: expected a non-empty list of patterns')
    return _checked([Pattern.from_dict(p) for p in d])


def _checked(patterns):
    patterns = list(patterns)
    if not 1 <= len(patterns) <= MAX_PATTERNS or not all(isinstance(p, Pattern) for p in patterns):
        raise ValueError(f'phoregen_amd.substructure: patterns must be 1 .. {MAX_PATTERNS} Pattern objects, not {len(patterns)} of '
                         f'{sorted({type(p).__name__ for p in patterns})}')
    names = [p.name for p in patterns]
    if len(set(names)) != len(names):
        raise ValueError(f'phoregen_amd.substructure: pattern names must be distinct, got {names}')
    return patterns


# ---- the table --------------------------------------------------------------------------------------------------------------------
def pattern_table(patterns):
    """The host table of pg_mol_sub: uint8 [P, PATTERN_BYTES] in the layout of include/phoregen_hip.h (PG_SUB_OFF_*)."""
    patterns = _checked(patterns)
    t = np.zeros((len(patterns), PATTERN_BYTES), dtype=np.uint8)
    for row, p in zip(t, patterns):
        row[hip.PG_SUB_OFF_K] = p.k
        row[hip.PG_SUB_OFF_MIN:hip.PG_SUB_OFF_MIN + 4] = np.frombuffer(np.int32(p.min).tobytes(), dtype=np.uint8)
        row[hip.PG_SUB_OFF_MAX:hip.PG_SUB_OFF_MAX + 4] = np.frombuffer(np.int32(-1 if p.max is None else p.max).tobytes(), dtype=np.uint8)
        row[hip.PG_SUB_OFF_ORDER:hip.PG_SUB_OFF_ORDER + p.k] = p.match_order
        for q, a in enumerate(p.atoms):
            rec = row[hip.PG_SUB_OFF_ATOMS + q * hip.PG_SUB_ATOM_BYTES:][:hip.PG_SUB_ATOM_BYTES]
            bits = sum(1 << c for c in a.elements)
            rec[hip.PG_SUB_ATOM_ELEMENTS], rec[hip.PG_SUB_ATOM_ELEMENTS + 1] = bits & 255, bits >> 8
            rec[hip.PG_SUB_ATOM_DEGREE], rec[hip.PG_SUB_ATOM_DEGREE + 1] = a.degree
            rec[hip.PG_SUB_ATOM_HCOUNT], rec[hip.PG_SUB_ATOM_HCOUNT + 1] = a.hcount
            charge = None if a.charge is None else a.charge == 1
            rec[hip.PG_SUB_ATOM_FLAGS] = _FLAG[charge] | _FLAG[a.ring] << 2 | _FLAG[a.aromatic] << 4
        for b in p.bonds:
            byte = sum(1 << (o - 1) for o in b.orders) | _FLAG[b.ring] << 4
            row[hip.PG_SUB_OFF_BONDS + b.a * MAX_ATOMS + b.b] = row[hip.PG_SUB_OFF_BONDS + b.b * MAX_ATOMS + b.a] = byte
    return t


def unpack_table(table, names=None):
    """The inverse of `pattern_table` (names are not part of a row: 'p0', 'p1', .. unless given)."""
    table = np.asarray(table, dtype=np.uint8).reshape(-1, PATTERN_BYTES)
    out = []
    for i, row in enumerate(table):
        k = int(row[hip.PG_SUB_OFF_K])
        lo = int(np.frombuffer(row[hip.PG_SUB_OFF_MIN:hip.PG_SUB_OFF_MIN + 4].tobytes(), dtype=np.int32)[0])
        hi = int(np.frombuffer(row[hip.PG_SUB_OFF_MAX:hip.PG_SUB_OFF_MAX + 4].tobytes(), dtype=np.int32)[0])
        atoms = []
        for q in range(k):
            rec = [int(v) for v in row[hip.PG_SUB_OFF_ATOMS + q * hip.PG_SUB_ATOM_BYTES:][:hip.PG_SUB_ATOM_BYTES]]
            bits, flags = rec[hip.PG_SUB_ATOM_ELEMENTS] | rec[hip.PG_SUB_ATOM_ELEMENTS + 1] << 8, rec[hip.PG_SUB_ATOM_FLAGS]
            charge = _FLAG_BACK[flags & 3]
            atoms.append(QueryAtom(tuple(c for c in range(N_CLASSES) if bits >> c & 1), (rec[hip.PG_SUB_ATOM_DEGREE], rec[hip.PG_SUB_ATOM_DEGREE + 1]),
                                   (rec[hip.PG_SUB_ATOM_HCOUNT], rec[hip.PG_SUB_ATOM_HCOUNT + 1]), None if charge is None else int(charge),
                                   _FLAG_BACK[flags >> 2 & 3], _FLAG_BACK[flags >> 4 & 3]))
        bonds = []
        for a in range(k):
            for b in range(a + 1, k):
                byte = int(row[hip.PG_SUB_OFF_BONDS + a * MAX_ATOMS + b])
                if byte:
                    bonds.append(QueryBond(a, b, tuple(o for o in (1, 2, 3, 4) if byte >> (o - 1) & 1), _FLAG_BACK[byte >> 4 & 3]))
        p = Pattern(names[i] if names is not None else f'p{i}', tuple(atoms), tuple(bonds), lo, None if hi < 0 else hi)
        if tuple(int(v) for v in row[hip.PG_SUB_OFF_ORDER:hip.PG_SUB_OFF_ORDER + k]) != p.match_order:
            raise _err(f'row {i}: the matching order in the table is not the breadth-first order {list(p.match_order)}')
        out.append(p)
    return out


# ---- the device call ---------------------------------------------------------------------------------------------------------------
@dataclass
class Substructure:
    """Device tensors of one `substructure` call; F frames, B graphs, P patterns."""
    embeddings: torch.Tensor     # int32 [F, B, P]     embeddings, saturating at 2**31 - 1
    anchors: torch.Tensor        # int32 [F, B, P]     distinct images of query atom 0
    atom_mask: torch.Tensor      # int64 [F, B, P, 2]  bit c of word c >> 6: the atom with compact index c lies in an embedding
    first: torch.Tensor          # int16 [F, B, P, 16] the first embedding per query atom (compact indices), -1 beyond k / without one
    status: torch.Tensor         # int32 [F, B, P]     SUB_* bits
    ok: torch.Tensor             # bool  [F, B]        no pattern of the graph has SUB_OUT_OF_BOUNDS
    patterns: list
    max_steps: int
    screen: M.Screen             # the screen it was computed from
    rings: M.Rings
    kekule: M.Kekule


def _check_steps(fn, max_steps):
    return M._check_int(f'phoregen_amd.substructure.{fn}', 'max_steps', max_steps, 1, MAX_STEPS)


@torch.no_grad()
def substructure(results, patterns, frames='final', screen=None, rings=None, kekule=None, max_steps=DEFAULT_STEPS):
    """Search every pattern in every decoded (frame, graph) of a `sample` / `sample_batch` result, on the device, in one launch
    (pg_mol_sub; DESIGN.md 2.9 "Substructure").  Whichever of `screen`, `rings` (a `Rings`) and `kekule` (a `Kekule`) is not handed
    in is computed; all must come from one screen.  No host read beyond the screen's.  max_steps bounds the partial embeddings
    tried per root; a (graph, pattern) that exceeds it gets SUB_TRUNCATED and lower bounds, every other row is exact."""
    patterns = _checked(patterns)
    max_steps = _check_steps('substructure', max_steps)
    node, _, _, F, _ = M._frames(results, frames)
    dev = node.device
    M._need_cuda('substructure', 'the substructure search', dev)
    sc = M._resolve('substructure', results, frames, screen, 'phoregen_amd.substructure', rings=rings, kekule=kekule)
    rg = rings if rings is not None else M.rings(results, frames, screen=sc)
    kek = kekule if kekule is not None else M.kekulize(results, frames, screen=sc)
    B, P = len(sc.num_atoms), len(patterns)
    with torch.cuda.device(dev):
        lib = hip.lib()
        host = pattern_table(patterns)
        table = torch.from_numpy(host).to(dev)
        out = dict(embeddings=torch.empty(F, B, P, dtype=torch.int32, device=dev), anchors=torch.empty(F, B, P, dtype=torch.int32, device=dev),
                   atom_mask=torch.empty(F, B, P, 2, dtype=torch.int64, device=dev),
                   first=torch.empty(F, B, P, MAX_ATOMS, dtype=torch.int16, device=dev), status=torch.empty(F, B, P, dtype=torch.int32, device=dev))
        _launch_sub(lib, sc, rg, kek, B, F, max(sc.num_atoms, default=0), table, host, P, max_steps, out)
    return Substructure(ok=((out['status'] & SUB_OUT_OF_BOUNDS) == 0).all(-1), patterns=patterns, max_steps=max_steps, screen=sc, rings=rg,
                        kekule=kek, **out)


def _launch_sub(lib, sc, rg, kek, B, F, max_n, table, table_host, P, max_steps, out):
    """pg_mol_sub on the current stream; sc, rg, kek: anything with the `Screen`, `Rings` and `Kekule` fields the kernel reads; table:
    uint8 [P, PATTERN_BYTES] on the device, table_host: the same bytes as a numpy array (the library checks the rows from it).  A
    graph above MAX_ATOMS, P or max_steps out of range or a malformed row is the library's error: nothing is launched and `out` is not
    written."""
    cls, order = sc.cls, sc.order
    M._check_arrays('substructure', cls.device, [
        (cls, torch.int8), (order, torch.int8), (sc.compact, torch.int16), (rg.ring_size, torch.uint8), (rg.atom_ring, torch.uint8),
        (kek.hcount, torch.uint8), (kek.charge, torch.int8), (kek.status, torch.int32), (sc.lig_off, torch.int32), (sc.bond_off, torch.int32),
        (table, torch.uint8), (out['embeddings'], torch.int32), (out['anchors'], torch.int32), (out['atom_mask'], torch.int64),
        (out['first'], torch.int16), (out['status'], torch.int32)])
    table_host = np.ascontiguousarray(table_host, dtype=np.uint8)
    rows = max(P, 0)
    if (sc.lig_off.numel() != B + 1 or sc.bond_off.numel() != B + 1 or cls.numel() != F * cls.size(-1) or order.numel() != F * order.size(-1)
            or sc.compact.shape != cls.shape or rg.atom_ring.shape != cls.shape or kek.hcount.shape != cls.shape
            or kek.charge.shape != cls.shape or rg.ring_size.shape != order.shape or kek.status.numel() != F * B
            or table.numel() < rows * PATTERN_BYTES or table_host.size < rows * PATTERN_BYTES
            or out['embeddings'].numel() < F * B * rows or out['anchors'].numel() < F * B * rows or out['status'].numel() < F * B * rows
            or out['atom_mask'].numel() < 2 * F * B * rows or out['first'].numel() < MAX_ATOMS * F * B * rows):
        raise ValueError(f'phoregen_amd.substructure.substructure: sizes of the offsets, screen / ring / Kekulé arrays, table and outputs do '
                         f'not fit {F} frames x {B} graphs x {P} patterns, {cls.size(-1)} atom rows, {order.size(-1)} pair rows')
    hip.check(lib.pg_mol_sub(cls.data_ptr(), order.data_ptr(), sc.compact.data_ptr(), rg.ring_size.data_ptr(), rg.atom_ring.data_ptr(),
                             kek.hcount.data_ptr(), kek.charge.data_ptr(), kek.status.data_ptr(), sc.lig_off.data_ptr(),
                             sc.bond_off.data_ptr(), B, F, cls.size(-1), 2 * order.size(-1), max_n, table.data_ptr(),
                             table_host.ctypes.data, P, max_steps, out['embeddings'].data_ptr(), out['anchors'].data_ptr(),
                             out['atom_mask'].data_ptr(), out['first'].data_ptr(), out['status'].data_ptr(), hip.stream_ptr()),
              'pg_mol_sub')


def status_names(status):
    return tuple(name for bit, name in SUB_NAMES.items() if status & bit)


def mask_atoms(words):
    """The compact indices of the set bits of an `atom_mask` row (two 64-bit patterns, signed or unsigned)."""
    return [w * 64 + b for w, v in enumerate(words) for b in range(64) if (int(v) & (1 << 64) - 1) >> b & 1]


# ---- the exact host enumerator ------------------------------------------------------------------------------------------------------
def _mol_properties(mol, pattern):
    """Per atom (class, degree, hcount, charge, in ring, aromatic) and {(a, b): (order, ring bond)} of one of `assemble`'s dicts.  The
    ring and Kekulé entries are read only if the pattern constrains them."""
    n = len(mol['element'])
    bi, bt = np.asarray(mol['bond_index']).reshape(2, -1), np.asarray(mol['bond_type']).reshape(-1)
    if pattern.uses_rings and 'rings' not in mol:
        raise ValueError(f'find_matches: pattern {pattern.name!r} constrains ring membership and the molecule carries no rings (assemble(rings=))')
    if pattern.uses_kekule and 'kekule' not in mol:
        raise ValueError(f'find_matches: pattern {pattern.name!r} constrains hydrogens or charge and the molecule carries no kekule '
                         '(assemble(kekule=))')
    ring_size = np.asarray(mol['rings']['bond_ring_size']).reshape(-1).tolist() if pattern.uses_rings else [0] * bt.size
    atom_ring = np.asarray(mol['rings']['atom_ring']).reshape(-1).tolist() if pattern.uses_rings else [0] * n
    h = np.asarray(mol['kekule']['hcount']).reshape(-1).tolist() if pattern.uses_kekule else [0] * n
    q = np.asarray(mol['kekule']['charge']).reshape(-1).tolist() if pattern.uses_kekule else [0] * n
    bonds, degree, aromatic = {}, [0] * n, [False] * n
    for a, b, t, r in zip(bi[0].tolist(), bi[1].tolist(), bt.tolist(), ring_size):
        bonds[(a, b)] = bonds[(b, a)] = (int(t), r > 0)
        for x in (a, b):
            degree[x] += 1
            aromatic[x] = aromatic[x] or t == 4
    atoms = [(ATOM_TYPES.index(int(z)), degree[i], int(h[i]), int(q[i]), atom_ring[i] > 0, aromatic[i]) for i, z in enumerate(mol['element'])]
    return atoms, bonds


def _atom_meets(a, prop):
    cls, degree, h, q, ring, arom = prop
    return (cls in a.elements and a.degree[0] <= degree <= a.degree[1] and a.hcount[0] <= h <= a.hcount[1]
            and (a.charge is None or a.charge == q) and (a.ring is None or a.ring == ring) and (a.aromatic is None or a.aromatic == arom))


def find_matches(mol, pattern, limit=None):
    """Every embedding of `pattern` in one of `assemble`'s dicts, exactly, on the host: a list of tuples, entry q the image of query
    atom q (an index into the dict's atoms), in the defined order -- by the images listed in matching order, lexicographically; the
    first entry is the kernel's `first`.  limit: stop after this many.  A pattern that constrains rings, hydrogens or charge needs a
    molecule assembled with rings= / kekule=; on a molecule that is not 'kekule_ok' such a pattern has no embedding.  No work bound."""
    if not isinstance(pattern, Pattern):
        raise ValueError(f'find_matches: pattern must be a Pattern, not {type(pattern).__name__}')
    atoms, bonds = _mol_properties(mol, pattern)
    if pattern.uses_kekule and not mol['kekule']['kekule_ok']:
        return []
    order, k = pattern.match_order, pattern.k
    qbond = {}
    for b in pattern.bonds:
        qbond[(b.a, b.b)] = qbond[(b.b, b.a)] = b
    back = [[(e, qbond[(order[d], order[e])]) for e in range(d) if (order[d], order[e]) in qbond] for d in range(k)]
    compat = [[t for t in range(len(atoms)) if _atom_meets(pattern.atoms[order[d]], atoms[t])] for d in range(k)]
    out, image = [], []

    def extend(d):
        if d == k:
            emb = [0] * k
            for pos, t in enumerate(image):
                emb[order[pos]] = t
            out.append(tuple(emb))
            return limit is not None and len(out) >= limit
        for t in compat[d]:
            if t in image:
                continue
            for e, qb in back[d]:
                tb = bonds.get((image[e], t))
                if tb is None or tb[0] not in qb.orders or (qb.ring is not None and qb.ring != tb[1]):
                    break
            else:
                image.append(t)
                stop = extend(d + 1)
                image.pop()
                if stop:
                    return True
        return False

    extend(0)
    return out


# ---- carriers (molecule.assemble / write_sdf) --------------------------------------------------------------------------------------
def molecule_entries(patterns, embeddings, anchors, atom_mask, first, status):
    """The 'substructure' dict of one molecule from its rows of the five outputs (host arrays, [P, ..]): pattern name -> 'embeddings',
    'anchors', 'atoms' (compact indices in an embedding), 'first' (the first embedding per query atom, None without one), 'status'
    (SUB_* bits) and 'status_names'."""
    out = {}
    for i, p in enumerate(patterns):
        f = [int(v) for v in first[i][:p.k]]
        st = int(status[i])
        out[p.name] = {'embeddings': int(embeddings[i]), 'anchors': int(anchors[i]), 'atoms': mask_atoms(atom_mask[i]),
                       'first': f if f and f[0] >= 0 else None, 'status': st, 'status_names': status_names(st)}
    return out


def sdf_item(entries):
    """The PHOREGEN_SUBSTRUCTURE data item: one line per pattern -- name, embeddings, anchors, status as hex, the atoms in an
    embedding and the first embedding as comma-separated 1-based atom numbers ('-' if empty)."""
    def numbers(v):
        return ','.join(str(a + 1) for a in v) if v else '-'
    lines = ['> <PHOREGEN_SUBSTRUCTURE>']
    lines += ['%s %d %d 0x%02x %s %s' % (name, e['embeddings'], e['anchors'], e['status'], numbers(e['atoms']), numbers(e['first']))
              for name, e in entries.items()]
    return '\n'.join(lines) + '\n\n'


def _molecule_entry(x, v, at, mol):
    """What a molecule carries: 'substructure', and 'substructure_ok' iff none of its patterns is SUB_OUT_OF_BOUNDS (`Substructure.ok`)."""
    entries = molecule_entries(x.patterns, *(at.row(v[name]) for name in ('u_emb', 'u_anchors', 'u_mask', 'u_first', 'u_status')))
    return {'substructure': entries, 'substructure_ok': all(not e['status'] & SUB_OUT_OF_BOUNDS for e in entries.values())}


def _read(value):
    """`sample_valid(substructure=)`: a list of patterns, or (patterns, max_steps)."""
    patterns, steps = value if isinstance(value, tuple) else (value, DEFAULT_STEPS)
    return _checked(patterns), _check_steps('sample_valid', steps)


ANALYSIS = M._Analysis(
    'substructure', 'substructure', Substructure, entry=_molecule_entry, sdf=lambda m: sdf_item(m['substructure']), read=_read,
    parts=lambda x: [('u_mask', x.atom_mask[0], np.int64), ('u_emb', x.embeddings[0], np.int32), ('u_anchors', x.anchors[0], np.int32),
                     ('u_status', x.status[0], np.int32), ('u_first', x.first[0], np.int16)],
    compute=lambda d, opt: substructure(d.res, opt[0], screen=d.screen, rings=d.of('rings'), kekule=d.of('kekule'), max_steps=opt[1]),
    verdict=lambda m: m['substructure_ok'])


def parse_sdf_item(text):
    """The inverse of `sdf_item` on the text of one SDF record: {} without the item."""
    if '> <PHOREGEN_SUBSTRUCTURE>\n' not in text:
        return {}
    out = {}
    for line in text.split('> <PHOREGEN_SUBSTRUCTURE>\n')[1].split('\n\n')[0].split('\n'):
        name, emb, anc, st, atoms, first = line.split()
        out[name] = {'embeddings': int(emb), 'anchors': int(anc), 'atoms': [] if atoms == '-' else [int(a) - 1 for a in atoms.split(',')],
                     'first': None if first == '-' else [int(a) - 1 for a in first.split(',')], 'status': int(st, 16),
                     'status_names': status_names(int(st, 16))}
    return out
