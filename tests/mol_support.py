"""What the molecule tests share (tests/*_reference.py, tests/test_mol*_host.py, tests/test_gpu_mol*.py), defined once: the element
classes, the builders of small graphs, the step from classes to pair rows and the one walk over them, the record of everything a
kernel reads for one graph, batches in the sampler's layout, the build and the calls of the host-check programs under tools/, the
split of a device result into graphs, and the readers of include/phoregen_hip.h and of V2000 blocks.  CPU only: nothing here needs a
device, and nothing here restates a kernel -- the restatements, their named molecules, families and tolerances live in the
*_reference.py modules, which import this one (never the other way round)."""
import os
import re
import subprocess
from typing import NamedTuple

import numpy as np
import torch

from mol_reference import pair_row, scores_from_classes
from phoregen_amd.plan import make_edge_data
from phoregen_amd.utils.sample_utils import ATOM_TYPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- names and constants ----------------------------------------------------------------------------------------------------------------
B_, C_, N_, O_, F_, SI_, P_, S_, CL_, BR_, I_ = range(11)           # the atom classes of the kept elements, in ATOM_TYPES' order
M64 = (1 << 64) - 1


# ---- graph builders: {(a, b): bond class} with a < b ------------------------------------------------------------------------------------
def cycle(n, order, off=0):
    return {(min(off + i, off + (i + 1) % n), max(off + i, off + (i + 1) % n)): order for i in range(n)}


def chain(n, order, off=0):
    return {(off + i, off + i + 1): order for i in range(n - 1)}


def mirrored(pos):
    """The mirror image: x -> -x.  An array of pos' own dtype (float64 for a list)."""
    return np.asarray(pos) * np.array([-1.0, 1.0, 1.0], dtype=np.asarray(pos).dtype)


def mol_dict(elements, bonds, types):
    """An assembled-style dict from atomic numbers, [(a, b)] and the bond types, coordinates made up."""
    n = len(elements)
    return {'element': list(elements), 'atom_pos': torch.arange(3 * n, dtype=torch.float32).reshape(n, 3) * 0.5 - 1.0,
            'bond_index': torch.tensor(bonds, dtype=torch.long).reshape(-1, 2).T, 'bond_type': torch.tensor(types, dtype=torch.long),
            'status': 0, 'valid': True}


# ---- from classes to rows, and the one walk over the rows -------------------------------------------------------------------------------
def rows_of(classes, bonds):
    """(cls, order) rows of one graph, as the screen would write them, from classes 0..11 and {(a, b): bond class 1..5}."""
    n = len(classes)
    cls = np.array([c if c <= 10 else -1 for c in classes], dtype=np.int8)
    order = np.zeros(n * (n - 1) // 2, dtype=np.int8)
    for (a, b), t in bonds.items():
        assert a < b
        if 1 <= t <= 4 and cls[a] >= 0 and cls[b] >= 0:
            order[pair_row(a, b, n)] = t
    return cls, order


class PairWalk(NamedTuple):
    kept: list                   # per atom: is its class one of the kept elements'
    nbrs: list                   # per atom: its neighbours, ascending
    rows: dict                   # {(a, b): pair row} of the bonds, a < b, in row order
    order: list                  # per pair row: the order handed in, as ints -- order[rows[(a, b)]] is the bond's


def pair_walk(cls, order, bonded=(1, 2, 3, 4)):
    """One graph as a kernel reads it: cls [n] (-1 = dropped), order [n (n - 1) / 2] for the pairs a < b in row-major order.  A pair
    is a bond if both atoms are kept and its order is one of `bonded`."""
    cls, order = [int(c) for c in cls], [int(o) for o in order]
    n = len(cls)
    kept = [0 <= c <= 10 for c in cls]
    nbrs, rows, row = [[] for _ in range(n)], {}, 0
    for a in range(n):
        for b in range(a + 1, n):
            if order[row] in bonded and kept[a] and kept[b]:
                nbrs[a].append(b), nbrs[b].append(a)                   # (ascending as they come: every a < x before every b > x)
                rows[(a, b)] = row
            row += 1
    assert row == len(order)
    return PairWalk(kept, nbrs, rows, order)


def compact_bonds(cls, order, bonded=(1, 2, 3, 4)):
    """(kept atoms' local indices, {(a, b): order} in the compact numbering of the kept atoms) of `pair_walk`'s bonds."""
    w = pair_walk(cls, order, bonded)
    kept = [i for i, k in enumerate(w.kept) if k]
    compact = {i: c for c, i in enumerate(kept)}
    return kept, {(compact[a], compact[b]): w.order[row] for (a, b), row in w.rows.items()}


class MolRows(NamedTuple):
    """Everything the kernels read for one graph; a field that a module does not compute is None."""
    cls: object
    order: object
    kekule_order: object
    hcount: object
    charge: object
    kekule_status: object
    ring_size: object = None
    colour: object = None
    key: object = None
    pos: object = None

    def smiles_inputs(self):
        """What the SMILES restatements take first: (cls, kekule_order, hcount, charge, kekule_status)."""
        return self.cls, self.kekule_order, self.hcount, self.charge, self.kekule_status


# ---- batches in the sampler's layout ----------------------------------------------------------------------------------------------------
def batch_from(graphs):
    """(node, pos, edge, sizes) as CPU tensors in the sampler's layout from [(atom classes 0..11, {(a, b): bond class 1..5})] or
    [(classes, bonds, pos [n, 3])], one-hot scores; without coordinates `scores_from_classes` makes them up."""
    parts = [scores_from_classes(list(g[0]), g[1], pos=torch.as_tensor(np.asarray(g[2], dtype=np.float32)).reshape(-1, 3) if len(g) > 2 else None)
             for g in graphs]
    return (torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts]), [len(g[0]) for g in graphs])


def renumbered_rows(p):
    """With atom i of a graph renumbered to p[i] (a numpy permutation): the pair row that every pair row, in order, moves to."""
    n = len(p)
    a, b = np.triu_indices(n, 1)
    lo, hi = np.minimum(p[a], p[b]), np.maximum(p[a], p[b])
    return lo * n - lo * (lo + 1) // 2 + (hi - lo - 1)


def mol_result(node, pos, edge, sizes, traj=(None, None, None), dev='cuda'):
    """A sampler-shaped result dict on the device; traj: the three trajectory tensors (a tensor already on the device is kept as it
    is, strides included) or None."""
    na = torch.tensor(sizes, dtype=torch.long)
    ei, eb = make_edge_data(na)
    return {'pred': [node.to(dev), pos.to(dev), edge.to(dev)], 'traj': [None if t is None else t.to(dev) for t in traj],
            'lig_info': [na.to(dev), torch.repeat_interleave(torch.arange(len(sizes)), na).to(dev), ei.to(dev), eb.to(dev)]}


def permute_batch(node, pos, edge, sizes, seed):
    """Every graph's atoms renumbered at random (atom i becomes perms[g][i]) and both halves of its bond rows moved to the rows of
    the renumbered pairs.  The kernel reads the first half only, so the pair's first-half scores stay in the first half whichever
    of its ends now has the smaller index."""
    rng = np.random.default_rng(seed)
    node2, pos2, edge2, perms = node.clone(), pos.clone(), edge.clone(), []
    n0, e0 = 0, 0
    for n in sizes:
        h = n * (n - 1) // 2
        p = rng.permutation(n)
        perms.append(p)
        dst = torch.from_numpy(n0 + p)
        node2[dst], pos2[dst] = node[n0:n0 + n], pos[n0:n0 + n]
        if h:
            rows = torch.from_numpy(renumbered_rows(p))
            assert sorted(rows.tolist()) == list(range(h))
            edge2[e0 + rows] = edge[e0:e0 + h]
            edge2[e0 + h + rows] = edge[e0 + h:e0 + 2 * h]
        n0, e0 = n0 + n, e0 + 2 * h
    return node2, pos2, edge2, perms


def onehot_graph(atom_cls, et_half):
    """One graph from atom classes [n] and first-half bond classes [h] (written to both halves), one-hot scores."""
    n, h = len(atom_cls), len(et_half)
    node = torch.zeros(n, 12)
    node[torch.arange(n), torch.as_tensor(atom_cls, dtype=torch.long)] = 1.0
    edge = torch.zeros(2 * h, 6)
    edge[torch.arange(2 * h), torch.as_tensor(np.concatenate([et_half, et_half]), dtype=torch.long)] = 1.0
    return node, torch.arange(3 * n, dtype=torch.float32).reshape(n, 3) * 0.25, edge


def cat_graphs(parts):
    return tuple(torch.cat([p[k] for p in parts]) for k in range(3))


# ---- the host-check programs under tools/: stand-alone, compiled with the sanitizers, run as child processes ----------------------------
def build_host_check(name, out_dir):
    """Compile tools/<name>.cpp with g++ under ASan + UBSan; returns the program's path."""
    exe = os.path.join(str(out_dir), name)
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    os.path.join(ROOT, 'tools', name + '.cpp'), '-o', exe], check=True)
    return exe


def run_program(exe, *args):
    """The lines of what the program wrote to its standard output; a non-zero exit status raises."""
    return subprocess.run([exe, *[str(a) for a in args]], check=True, capture_output=True, text=True).stdout.split('\n')


def hex32(x):
    """The value rounded to fp32, as hexadecimal text that a C program reads back exactly."""
    return float(np.float32(x)).hex()


def listed_pairs(n, *orders):
    """(rows, a, b) of a graph of n atoms: the pair rows at which any of the [n (n - 1) / 2] arrays is not 0, ascending, and the
    atoms a < b of those rows."""
    rows = np.nonzero(np.any([np.asarray(o) != 0 for o in orders], axis=0))[0]
    a, b = np.triu_indices(n, 1)
    return rows, a[rows], b[rows]


def padded_valences(table):
    """{atomic number: valences} as one flat list over ATOM_TYPES, every element padded with 0 to four entries."""
    return sum((list(table[z]) + [0] * (4 - len(table[z])) for z in ATOM_TYPES), [])


# ---- a device result per graph ----------------------------------------------------------------------------------------------------------
def split_frame(sizes, f=0, per_atom=None, per_pair=None, per_graph=None):
    """Frame f of tensors [F, ...] given by name, as one dict of numpy values per graph: a per_atom tensor [F, N, ...] cut to the
    graph's n atoms, a per_pair tensor [F, H, ...] to its n (n - 1) / 2 pair rows, a per_graph tensor [F, B, ...] to its row -- as a
    Python number where the row is a single one."""
    atoms, pairs, graphs = ({k: t[f].cpu().numpy() for k, t in (d or {}).items()} for d in (per_atom, per_pair, per_graph))
    out, n0, h0 = [], 0, 0
    for g, n in enumerate(sizes):
        h = n * (n - 1) // 2
        r = {k: v[n0:n0 + n] for k, v in atoms.items()}
        r.update((k, v[h0:h0 + h]) for k, v in pairs.items())
        r.update((k, v[g].item() if v.ndim == 1 else v[g]) for k, v in graphs.items())
        out.append(r)
        n0, h0 = n0 + n, h0 + h
    return out


def bits(x):
    """A value in a form whose `==` is equality bit for bit (NaNs included): a float32 tensor as integers of its own width, an
    array as its bytes, anything else as it is."""
    if isinstance(x, torch.Tensor):
        return x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x
    return x.tobytes() if isinstance(x, np.ndarray) else x


# ---- include/phoregen_hip.h and V2000 blocks --------------------------------------------------------------------------------------------
_HEADER = []


def header_text():
    """include/phoregen_hip.h, read once."""
    if not _HEADER:
        with open(os.path.join(ROOT, 'include', 'phoregen_hip.h')) as fh:
            _HEADER.append(fh.read())
    return _HEADER[0]


def header_macro(name):
    """The text that `#define <name>` gives the macro in the header; None if the header does not define it."""
    m = re.search(r'#define %s (\S+)' % re.escape(name), header_text())
    return m and m.group(1)


def arg_count(name):
    """The number of arguments of the header's declaration `int <name>(...)`, comments taken out."""
    return re.sub(r'/\*.*?\*/', '', header_text().split('int %s(' % name)[1].split(');')[0]).count(',') + 1


def read_mol_block(text):
    """A small V2000 reader: ([(symbol, x, y, z)], [(a, b, type)]) with 0-based atoms."""
    lines = text.split('\n')
    na, nb = int(lines[3][0:3]), int(lines[3][3:6])
    atoms = [(ln[31:34].strip(), float(ln[0:10]), float(ln[10:20]), float(ln[20:30])) for ln in lines[4:4 + na]]
    bonds = [(int(ln[0:3]) - 1, int(ln[3:6]) - 1, int(ln[6:9])) for ln in lines[4 + na:4 + na + nb]]
    assert lines[4 + na + nb].startswith('M  ') and lines[3].endswith('V2000')
    return atoms, bonds
