"""Writes tests/golden/distance_bonds_v1.npz: what the reference's own utils/predict_bonds.py answers, recorded for the tests of the
distance bond screen (phoregen_amd.molecule.screen(bonds='distance'); tests/test_molbonds_host.py, tests/test_gpu_molbonds.py).

The reference file is loaded by path (it needs numpy only); nothing of its text is kept, only what it returns:
  table_pairs [66, 2], table_lengths [66, 3]: for every unordered pair of the project's eleven elements (atomic numbers, lower first)
      the single / double / triple length in pm that the reference's lookup finds for it (lower atomic number first, as
      `predict_bonds` sorts a pair), 0 where it finds none.
  sizes [M], elements [sum], pos [sum, 3] fp32: M molecules of 1..60 atoms over the nine elements the reference can name (grown
      chains and rings with bond lengths across 1.0 .. 2.3 Angstrom, and loose clouds), and for each
  bond_off [M + 1], bond_index [2, sum], bond_type [sum]: `predict_bonds(elements, pos)` as returned, both directions.
Two conditions are asserted before the file is written: no pair lies within MARGIN_PM of a threshold of its two elements (float64 on
the fp32 coordinates; tests/bonds_reference.py says why that makes every later comparison exact), and the recorded answer holds at
least 50 bonds of each order.

    python tools/make_distance_bond_golden.py            (the reference at $PHOREGEN_REFERENCE, see oracle/ref_import.py)"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import bonds_reference as BR                                # noqa: E402
from oracle import ref_import                               # noqa: E402
from phoregen_amd import molecule as M                      # noqa: E402
from phoregen_amd.utils.sample_utils import ATOM_TYPES      # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'distance_bonds_v1.npz')
SEED, MOLECULES, CENSUS_MIN = 20240914, 64, 50
MAPPED = [z for z in ATOM_TYPES if z not in (5, 14)]       # the reference's `periodic_table` literal loses B and Si
MAPPED_P = np.array([50, 14, 14, 4, 4, 6, 3, 3, 2]) / 100.0


def load_reference():
    spec = importlib.util.spec_from_file_location('reference_predict_bonds', os.path.join(ref_import.REFERENCE, 'utils', 'predict_bonds.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def table_dump(ref):
    pairs, lengths = [], []
    for i, z1 in enumerate(ATOM_TYPES):
        for z2 in ATOM_TYPES[i:]:
            s1, s2 = M.ELEMENT_SYMBOL[z1], M.ELEMENT_SYMBOL[z2]
            pairs.append((z1, z2))
            lengths.append([d.get(s1, {}).get(s2, 0) for d in (ref.bonds1, ref.bonds2, ref.bonds3)])
    return np.array(pairs, dtype=np.int16), np.array(lengths, dtype=np.int16)


def molecule(rng, g, n, thresholds):
    """Classes (ATOM_TYPES indices) and fp32 coordinates of molecule g."""
    cls = np.array([ATOM_TYPES.index(z) for z in rng.choice(MAPPED, size=n, p=MAPPED_P)])
    kind = g % 4

    def chain(i, placed):                                  # a bond of 1.0 .. 2.3 Angstrom to one of the last three atoms
        return placed[int(rng.integers(max(0, i - 3), i))] + rng.uniform(1.0, 2.3) * BR.unit(rng) if i else np.zeros(3)

    ring_n = int(rng.integers(3, 9))
    side = rng.uniform(1.0, 1.7)

    def ring(i, placed):                                   # a jittered regular polygon of `ring_n` atoms, then a chain
        if i >= ring_n:
            return chain(i, placed)
        r = side / (2.0 * np.sin(np.pi / ring_n))
        return np.array([r * np.cos(2 * np.pi * i / ring_n), r * np.sin(2 * np.pi * i / ring_n), 0.0]) + rng.normal(0, 0.03, 3)

    spread = 1.1 * max(n, 2) ** (1.0 / 3.0)
    propose = (chain, ring, chain, lambda i, placed: rng.normal(0, spread, 3))[kind]
    far = 0.95 if kind < 3 else 0.6                        # nothing but the partner closer than this (a few tries, then anything)
    pos = BR.place_atoms(cls, propose, thresholds, lambda i, c, placed: np.sort(np.sqrt(((placed - c) ** 2).sum(1)))[:2][-1] > far
                         if len(placed) > 1 else True, tries=30)
    return cls, pos


def main():
    ref = load_reference()
    rng = np.random.default_rng(SEED)
    thresholds = M.bond_thresholds()
    sizes = [1, 2, 3, 60] + [int(v) for v in rng.integers(4, 61, MOLECULES - 4)]
    elements, poss, bi, bt, off = [], [], [], [], [0]
    for g, n in enumerate(sizes):
        cls, pos = molecule(rng, g, n, thresholds)
        assert pos.dtype == np.float32 and BR.min_margin_pm(cls, pos, thresholds) >= BR.MARGIN_PM, (g, n)
        z = [ATOM_TYPES[c] for c in cls]
        index, types = ref.predict_bonds(z, pos)
        index = np.array(index, dtype=np.int16).reshape(2, -1)
        elements.append(np.array(z, dtype=np.int16)), poss.append(pos), bi.append(index), bt.append(np.array(types, dtype=np.int8))
        off.append(off[-1] + len(types))
    bond_type = np.concatenate(bt)
    census = np.bincount(bond_type, minlength=4) // 2
    print('molecules', len(sizes), 'atoms', sum(sizes), 'bonds of order 1 / 2 / 3:', census[1:].tolist())
    assert (census[1:4] >= CENSUS_MIN).all() and census.size == 4, census
    pairs, lengths = table_dump(ref)
    np.savez_compressed(OUT, table_pairs=pairs, table_lengths=lengths, sizes=np.array(sizes, dtype=np.int16),
                        elements=np.concatenate(elements), pos=np.concatenate(poss), bond_off=np.array(off, dtype=np.int32),
                        bond_index=np.concatenate(bi, axis=1), bond_type=bond_type, margin_pm=np.float64(BR.MARGIN_PM),
                        census_min=np.int32(CENSUS_MIN))
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')
    assert os.path.getsize(OUT) < 256 * 1024


if __name__ == '__main__':
    main()
