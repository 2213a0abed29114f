#!/usr/bin/env python3
"""Thin sampling driver with sample_all.py's flags (the reference's script cannot travel to the GPU box and its
RDKit/OpenBabel post-processing is out of scope): .phore files -> PhoreDiff.sample -> decode_batch -> per-molecule
element / position / bond arrays (.pt), the input of the reference's reconstruct_from_generated_with_edges.

  python tools/sample_cli.py --phore_file_list files.json --num_samples 100 --batch_size 30 --outdir results/x

--valid_only keeps sampling until --num_samples molecules have passed the device-side screen (one connected molecule, no atom
above its largest valence; phoregen_amd/molecule.py) and prints sample_all.py's `Finished n | Failed m` line; --sdf writes one V2000
.sdf per molecule as sample_all.py names them, <outdir>/sdf_results/{pidx}_{name}_{i}.sdf.  --unique (implies --valid_only) finishes
a molecule only if it is new: repeats, judged by the identity key and confirmed exactly (phoregen_amd.molecule.same_molecule), are
counted apart; <outdir>/{name}_keys.txt then lists one 16-digit hex key per finished molecule (the part sample_all.py's
{name}_SMILES_all.txt plays) and the .sdf files carry the key as a data item.  --geometry (implies --valid_only) also measures every
molecule against the pharmacophore it was generated for (phoregen_amd.molecule.geometry_for: bond lengths, clashes, clearance from the
exclusion spheres, features with an atom nearby) and finishes it only if no limit is broken; --geom_limits '{"bond_max": 2.2}' replaces
single limits of phoregen_amd.molecule.GeomLimits; the .sdf files carry the figures as a data item.  --rings (implies --valid_only)
also perceives the rings of every molecule (phoregen_amd.molecule.rings: smallest ring through every bond and atom, ring systems,
rotatable bonds, aromatic bonds outside a ring) and finishes it only if no ring limit is broken; with the default limits that is the
aromatic rule alone, --ring_limits '{"ring_min": 5, "ring_max": 8}' replaces single limits of phoregen_amd.molecule.RingLimits; the
.sdf files carry the counts as a data item.  --kekule (implies --valid_only) also resolves the aromatic bonds into single and double
bonds and gives every atom its hydrogens and charge (phoregen_amd.molecule.kekulize), and finishes a molecule only if it has such a
Kekulé structure; --no_charged forbids the N+ / P+ / S+ structures tried when no neutral one exists; with --sdf the blocks are then
written in Kekulé form with charges, and carry formula, weight and counts as the data item PHOREGEN_KEKULE.  --features (implies
--valid_only) also types every atom (HD, AR, PO, HA, HY, NE, XB; phoregen_amd.molecule.features_for) and matches every typed feature
point of the pharmacophore against the atoms that carry its type, and finishes a molecule only if it has a Kekulé structure to type
from and no more typed points are unmatched than --feature_limits '{"max_unmatched": 0}' allows (default: any number); the .sdf files
carry the counts and the per-point matches as the data item PHOREGEN_FEATURES.  --smiles (implies --valid_only) also writes every
molecule as Kekulé-form OpenSMILES text (phoregen_amd.molecule.smiles; with --no_charged from the neutral-only Kekulé form, as with --kekule) and finishes a molecule only if it
has a Kekulé structure to write from; <outdir>/{name}_SMILES_all.txt then holds one line per finished molecule, in the order of the
.sdf files -- the file sample_all.py writes -- and the .sdf files carry the text as the data item PHOREGEN_SMILES.  The text is not
canonical: a reader's own toolkit canonicalises it.  --stereo (implies --valid_only) also reads the stereo of every molecule from its
coordinates (phoregen_amd.molecule.stereo: tetrahedral centres, cis / trans double bonds outside rings) and finishes it only if it has a
Kekulé structure and finite coordinates; with --smiles the lines are then isomeric SMILES ('@', '@@', '/', '\\'), with --unique
stereoisomers count as different molecules and {name}_keys.txt lists the stereo keys, and the .sdf files carry the parities and labels
as the data item PHOREGEN_STEREO; --stereo_limits '{"vol_min": 0.6, "planar_min": 0.3, "max_undefined": 0}' replaces single limits
of phoregen_amd.molecule.StereoLimits.  --fingerprints (implies --valid_only) also gives every finished molecule its 2048-bit circular
fingerprint (phoregen_amd.molecule.fingerprints; --fp_radius R, 0 .. 4, default 2; not RDKit's ECFP) and compares the finished set on the
device (phoregen_amd.similarity): <outdir>/{name}_fingerprints.npy holds them as uint64 [n, 32] in the order of the finished molecules,
<outdir>/{name}_similarity.txt one line 'n internal_diversity mean_nearest_similarity', and the .sdf files carry the bits as the data
item PHOREGEN_FINGERPRINT.  --diverse K (implies --fingerprints) writes <outdir>/{name}_diverse.txt: the MaxMin picks from the first
finished molecule on, one line 'index pick_sim' per pick in pick order (at most n of them).  --reference_fps FILE.npy (uint64 [m, 32],
e.g. another run's {name}_fingerprints.npy; implies --fingerprints) writes <outdir>/{name}_nearest.txt: per finished molecule the
largest similarity to that set and the row that attains it.  --substructure patterns.json (implies --valid_only; the format is that
of tools/patterns/example_patterns.json, phoregen_amd.substructure.Pattern.from_dict) searches every pattern in every molecule on the
device and finishes a molecule only if, for every pattern, the number of anchors lies within the pattern's min / max;
<outdir>/{name}_substructure.txt holds one line 'index name embeddings anchors status' per finished molecule and pattern and the .sdf
files carry the data item PHOREGEN_SUBSTRUCTURE; --substructure_steps N replaces the work bound per root (default 65536).
--add_edge distance (the reference driver's spelling; implies --valid_only) takes the bonds from the sampled coordinates instead of the
bond scores (phoregen_amd.molecule.screen(bonds='distance')): validity and every analysis above then run on those bonds; 'openbabel' is
refused.  --bond_agreement (implies --valid_only) writes <outdir>/{name}_bond_agreement.txt, one line 'index mode both_same
both_aromatic both_differ predicted_only distance_only neither' per finished molecule, and the .sdf files carry the data item
PHOREGEN_BONDS.  --hydrogens (implies --valid_only and the Kekulé form) also gives every hydrogen its coordinates
(phoregen_amd.hydrogens: ideal local geometry, no force field) and finishes a molecule only if it has a Kekulé structure, finite
coordinates and no more contacts than allowed; with --sdf the blocks are then all-atom blocks and carry the counts as the data item
PHOREGEN_HYDROGENS; --hydrogen_options '{"clash_min": 1.2, "max_contacts": 0}' replaces single options of
phoregen_amd.hydrogens.HydrogenOptions.  --scaffolds (implies --valid_only) takes the finished molecules back to the device
(phoregen_amd.scaffold.batch_of) and writes the Murcko scaffold of each (phoregen_amd.scaffold.scaffolds: ring systems and linkers, with
the atoms double-bonded to them; --scaffold_plain leaves those out) and its generic framework (every atom carbon, every bond single):
<outdir>/{name}_scaffolds.txt holds one line 'index scaffold_key framework_key group scaffold_atoms ring_systems smiles' per finished
molecule -- the keys as 16 hex digits, group = the index of the first molecule with the same scaffold (confirmed exactly), the
scaffold's Kekulé-form SMILES or '-' without one -- and <outdir>/{name}_scaffold_summary.txt the lines 'molecules', 'distinct_scaffolds',
'distinct_frameworks', 'without_scaffold' and 'largest_group'.  --max_per_scaffold K (implies --scaffolds) writes
<outdir>/{name}_scaffold_picks.txt: the indices of the first K molecules of every scaffold, ascending.  --properties (implies
--valid_only) computes the property descriptors of every molecule on the device (phoregen_amd.properties: weight, the table sums tpsa,
logp and mr, the Lipinski and Veber counts, fsp3; the shipped tables are written from memory, not checked against RDKit) and finishes
a molecule only if it has a Kekulé structure and keeps the limits; --property_limits '{"preset": "lipinski"}' (or "veber"), or explicit
keys of phoregen_amd.properties.PropertyLimits such as '{"mol_weight": [null, 450], "sums": {"logp": [null, 4]}, "max_violations": 0}',
sets them (default: none).  <outdir>/{name}_properties.txt holds one line 'index mol_weight tpsa logp mr nhoh no_count rotatable
heavy_atoms fsp3 status' per finished molecule and the .sdf files carry the data item PHOREGEN_PROPERTIES.  --shape (implies
--valid_only) compares the finished molecules in space, where they lie in the pharmacophore's frame (phoregen_amd.shape: Gaussian-volume
overlap with no alignment; the radii are design choices, the values are not ROCS's): <outdir>/{name}_shape.txt holds one line 'index
volume nearest_sim nearest_index' per finished molecule -- volume = the molecule's self overlap in cubic Angstrom, the nearest other
finished molecule by shape Tanimoto -- and <outdir>/{name}_shape_summary.txt the lines 'molecules', 'internal_shape_diversity' and
'mean_nearest_shape_similarity'.  --shape_colour (needs --shape, implies --features) gives the set the atoms' feature types as colour and
scores by (1 - W) shape + W colour Tanimoto, W = --shape_colour_weight (default 0.5).  --shape_reference FILE.sdf (implies --shape)
reads the first mol block of the file, e.g. the ligand the pharmacophore was derived from, which must lie in the .phore file's frame:
every line gets the column 'reference_shape_sim' (shape only) and the summary the line 'mean_reference_shape_similarity'.
--shape_align (needs --shape --shape_reference) searches the best rigid overlay of the reference onto every finished molecule
(phoregen_amd.shape.align: five local ascents of the score; neither the definition nor the values are ROCS's or RDKit's), so the
reference may lie in any frame: every line gets 'aligned_shape_sim aligned_start' (the winning start, 0 in place, 1 .. 4 inertial) and
with --shape_colour 'aligned_colour_sim aligned_score', the summary 'mean_aligned_reference_shape_similarity'; --shape_align_sdf
(implies --shape_align) writes every finished molecule overlaid onto the reference under <outdir>/sdf_aligned/.  --num_steps shortens the reverse process (default: the model's).  Without them
nothing changes.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from phoregen_amd.config import default_model_config, load_config  # noqa: E402
from phoregen_amd.data import PHORETYPES1, parse_phore_file  # noqa: E402
from phoregen_amd.fragment import load_fragment_json  # noqa: E402
from phoregen_amd.models.diffusion import PhoreDiff  # noqa: E402
from phoregen_amd import scaffold as scaffold_mod  # noqa: E402
from phoregen_amd import shape as shape_mod  # noqa: E402
from phoregen_amd import similarity  # noqa: E402
from phoregen_amd import substructure as substruct  # noqa: E402
from phoregen_amd.hydrogens import HydrogenOptions  # noqa: E402
from phoregen_amd.properties import DEFAULT_TABLES, PropertyLimits  # noqa: E402
from phoregen_amd.molecule import BOND_AGREE_COUNTS, FP_MAX_RADIUS, FP_RADIUS, FP_WORDS, FeatureLimits, GeomLimits, KekuleOptions, RingLimits, StereoLimits, STATUS_NONFINITE, assemble, molecule_keys, point_kinds_of, sample_valid, screen, smiles, write_sdf  # noqa: E402
from phoregen_amd.utils.sample_utils import decode_batch  # noqa: E402
from phoregen_amd.weights import init_deterministic_  # noqa: E402


def property_limits_of(spec):
    """A PropertyLimits from the JSON object of --property_limits: {"preset": "lipinski" | "veber"} or keys of PropertyLimits, a
    (min, max) pair as a list with null for none."""
    spec = dict(spec or {})
    if 'preset' in spec:
        if set(spec) != {'preset'} or spec['preset'] not in ('lipinski', 'veber'):
            raise ValueError('--property_limits: "preset" stands alone and is "lipinski" or "veber"')
        return getattr(PropertyLimits, spec['preset'])()
    pair = lambda v: tuple(v) if isinstance(v, list) else v            # noqa: E731
    sums = {k: pair(v) for k, v in (spec.pop('sums', None) or {}).items()}
    return PropertyLimits(sums=sums, **{k: pair(v) for k, v in spec.items()})


def write_property_file(outdir, name, done):
    """<name>_properties.txt for the finished molecules (they carry 'properties' of the default tables): a header line, then one
    line 'index mol_weight tpsa logp mr nhoh no_count rotatable heavy_atoms fsp3 status' per molecule."""
    names = [t.name for t in DEFAULT_TABLES]
    with open(os.path.join(outdir, name + '_properties.txt'), 'w') as fh:
        fh.write('# index mol_weight ' + ' '.join(names) + ' nhoh no_count rotatable heavy_atoms fsp3 status\n')
        fh.writelines('%d %.3f %s %d %d %d %d %.4f 0x%02x\n' % (i, q['mol_weight'], ' '.join('%.4f' % q[k] for k in names), q['nhoh'], q['no_count'],
                                                                q['rotatable'], q['heavy_atoms'], q['fsp3'], q['status'])
                      for i, q in enumerate(m['properties'] for m in done))


def write_scaffold_files(outdir, name, done, exocyclic, max_per_scaffold):
    """<name>_scaffolds.txt, <name>_scaffold_summary.txt and, with max_per_scaffold, <name>_scaffold_picks.txt for the finished
    molecules: batch_of -> screen -> scaffolds as given and generic, keys of both, SMILES of the scaffold screen."""
    n = len(done)
    lines, group, sizes = [], torch.zeros(0, dtype=torch.long), torch.zeros(0, dtype=torch.long)
    if n:
        res = scaffold_mod.batch_of(done, 'cuda')
        sc = screen(res)
        sf = scaffold_mod.scaffolds(sc, scaffold_mod.ScaffoldOptions(exocyclic=exocyclic))
        fw = scaffold_mod.scaffolds(sc, scaffold_mod.ScaffoldOptions(exocyclic=exocyclic, generic=True))
        key, fkey = scaffold_mod.scaffold_keys(sf).key[0], molecule_keys(fw.screen).key[0]
        text = smiles(res, screen=sf.screen)
        group, sizes = scaffold_mod.scaffold_groups(key, assemble(res, screen=sf.screen))
        counts, ok = sf.counts[0].tolist(), text.ok[0].tolist()
        for i, (k, f, g, c, t) in enumerate(zip(key.tolist(), fkey.tolist(), group.tolist(), counts, text.strings())):
            lines.append('%d %016x %016x %d %d %d %s\n' % (i, k & (1 << 64) - 1, f & (1 << 64) - 1, g, c[0], c[6], t if ok[i] and t else '-'))
    with open(os.path.join(outdir, name + '_scaffolds.txt'), 'w') as fh:
        fh.writelines(lines)
    with open(os.path.join(outdir, name + '_scaffold_summary.txt'), 'w') as fh:
        fh.write('molecules: %d\ndistinct_scaffolds: %d\ndistinct_frameworks: %d\nwithout_scaffold: %d\nlargest_group: %d\n'
                 % (n, len(set(group.tolist())), len({ln.split()[2] for ln in lines}), sum(int(ln.split()[4]) == 0 for ln in lines),
                    int(sizes.max()) if n else 0))
    if max_per_scaffold is not None:
        with open(os.path.join(outdir, name + '_scaffold_picks.txt'), 'w') as fh:
            fh.writelines('%d\n' % i for i in scaffold_mod.pick_per_scaffold(group, max_per_scaffold).tolist())


def first_mol_block_of(text):
    """The first mol block of the text of an .sdf file: everything up to and including its 'M  END' line."""
    end = text.find('M  END')
    if end < 0:
        raise ValueError('no mol block (no "M  END" line)')
    return text[:end + len('M  END')] + '\n'


def write_shape_files(outdir, name, done, colour, weight, reference, align=False):
    """<name>_shape.txt and <name>_shape_summary.txt for the finished molecules: from_molecules -> nearest / internal_diversity, and
    with `reference` (a mol block) the shape Tanimoto to it.  colour: the molecules carry 'features' and the score is the combined one.
    align (needs `reference`): the best rigid overlay of the reference onto every molecule (`shape.align`) adds the columns
    'aligned_shape_sim aligned_start' -- with colour also 'aligned_colour_sim aligned_score'; the reference carries no colour, so its
    colour Tanimoto is 0 -- and the summary line 'mean_aligned_reference_shape_similarity'.  Returns the `ShapeAlignment` (None
    without align or without molecules): its transform moves the reference onto molecule i."""
    n, w = len(done), weight if colour else 0.0
    lines, diversity, mean_near, mean_ref, mean_aligned, overlay = [], float('nan'), float('nan'), float('nan'), float('nan'), None
    if n:
        mols = done if colour else [{'element': m['element'], 'atom_pos': m['atom_pos']} for m in done]
        st = shape_mod.from_molecules(mols, 'cuda')
        near = shape_mod.nearest(st, colour_weight=w)
        cols = [st.self_shape.tolist(), near.sim.tolist(), near.index.tolist()]
        if reference is not None:
            ref_set = shape_mod.from_mol_block(reference, 'cuda')
            ref = shape_mod.nearest(st, ref_set)
            cols.append(ref.sim.tolist())
            mean_ref = ref.sim.double().mean().item()
        diversity = shape_mod.internal_diversity(st, colour_weight=w)
        mean_near = near.sim.double().mean().item() if n >= 2 else float('nan')
        lines = ['%d %.3f %.6f %d' % (i, *row[:3]) + (' %.6f' % row[3] if reference is not None else '') for i, row in enumerate(zip(*cols))]
        if align:
            overlay = shape_mod.align(st, ref_set, colour_weight=w)
            mean_aligned = overlay.shape.double().mean().item()
            extra = zip(overlay.shape.tolist(), overlay.start.tolist(), overlay.colour.tolist(), overlay.score.tolist())
            lines = [ln + ' %.6f %d' % (s, k) + (' %.6f %.6f' % (c, f) if colour else '') for ln, (s, k, c, f) in zip(lines, extra)]
        lines = [ln + '\n' for ln in lines]
    with open(os.path.join(outdir, name + '_shape.txt'), 'w') as fh:
        fh.write('# index volume nearest_sim nearest_index' + (' reference_shape_sim' if reference is not None else '')
                 + (' aligned_shape_sim aligned_start' + (' aligned_colour_sim aligned_score' if colour else '') if align else '') + '\n')
        fh.writelines(lines)
    with open(os.path.join(outdir, name + '_shape_summary.txt'), 'w') as fh:
        fh.write('molecules: %d\ninternal_shape_diversity: %.6f\nmean_nearest_shape_similarity: %.6f\n' % (n, diversity, mean_near))
        if reference is not None:
            fh.write('mean_reference_shape_similarity: %.6f\n' % mean_ref)
        if align:
            fh.write('mean_aligned_reference_shape_similarity: %.6f\n' % mean_aligned)
    return overlay


def overlaid_onto_reference(m, rotation, translation):
    """The molecule moved by the inverse of (R, t), the transform that puts the reference onto it: x -> R^T (x - t), hydrogens
    included.  float64 on the host."""
    r, t = np.asarray(rotation, dtype=np.float64), np.asarray(translation, dtype=np.float64)
    move = lambda x: torch.as_tensor((np.asarray(x, dtype=np.float64).reshape(-1, 3) - t) @ r, dtype=torch.float32)     # noqa: E731
    out = dict(m, atom_pos=move(m['atom_pos']))
    if 'hydrogens' in m and 'h_pos' in m['hydrogens']:
        out['hydrogens'] = dict(m['hydrogens'], h_pos=move(m['hydrogens']['h_pos']))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', type=str, default=None, help='reference YAML (model: block); default = shipped values')
    ap.add_argument('--num_samples', type=int, default=100)
    ap.add_argument('--batch_size', type=int, default=30)
    ap.add_argument('--outdir', type=str, default='./results/test')
    ap.add_argument('--check_point', type=str, default=None, help="torch checkpoint with a 'model' state_dict")
    ap.add_argument('--phore_file_list', type=str, required=True, help='json list of .phore files')
    ap.add_argument('--pos_guidance_opt', type=json.loads, default=None)
    ap.add_argument('--sample_nodes_mode', type=str, default='uniform')
    ap.add_argument('--normal_scale', type=float, default=4.0)
    ap.add_argument('--seed', type=int, default=2032)
    ap.add_argument('--rng', type=str, default='device', choices=['device', 'cpu'])
    ap.add_argument('--fragment', type=str, default=None,
                    help="JSON file {'element' | 'type', 'pos', 'bonds'}: a fragment kept as the first atoms of every molecule "
                         '(world coordinates of the .phore frame; device RNG only)')
    ap.add_argument('--valid_only', action='store_true',
                    help='sample until num_samples molecules have passed the screen (give up after 3 * num_samples failures)')
    ap.add_argument('--unique', action='store_true',
                    help='implies --valid_only: a repeat of a finished molecule is not finished (also give up after 3 * num_samples repeats)')
    ap.add_argument('--geometry', action='store_true',
                    help='implies --valid_only: a molecule that breaks a geometry limit against its pharmacophore is not finished')
    ap.add_argument('--geom_limits', type=json.loads, default=None, help='JSON object replacing single limits of GeomLimits (with --geometry)')
    ap.add_argument('--rings', action='store_true',
                    help='implies --valid_only: a molecule that breaks a ring limit (default: an aromatic bond outside a ring) is not finished')
    ap.add_argument('--ring_limits', type=json.loads, default=None, help='JSON object replacing single limits of RingLimits (with --rings)')
    ap.add_argument('--kekule', action='store_true',
                    help='implies --valid_only: a molecule without a Kekulé structure is not finished; .sdf blocks are written in Kekulé form')
    ap.add_argument('--no_charged', action='store_true', help='with --kekule: neutral Kekulé structures only (no N+ / P+ / S+)')
    ap.add_argument('--features', action='store_true',
                    help='implies --valid_only: a molecule without a Kekulé structure, or with more unmatched typed feature points than '
                         '--feature_limits allows, is not finished')
    ap.add_argument('--feature_limits', type=json.loads, default=None,
                    help='JSON object replacing single limits of FeatureLimits (with --features), e.g. \'{"max_unmatched": 0}\'')
    ap.add_argument('--smiles', action='store_true',
                    help='implies --valid_only: a molecule without a Kekulé structure is not finished; writes <outdir>/<name>_SMILES_all.txt')
    ap.add_argument('--stereo', action='store_true',
                    help='implies --valid_only: reads centres and cis / trans double bonds from the coordinates; isomeric SMILES with --smiles, '
                         'stereoisomers apart with --unique')
    ap.add_argument('--stereo_limits', type=json.loads, default=None,
                    help='JSON object replacing single limits of StereoLimits (with --stereo): vol_min, planar_min, max_undefined')
    ap.add_argument('--fingerprints', action='store_true',
                    help='implies --valid_only: writes <outdir>/<name>_fingerprints.npy and <name>_similarity.txt (n, internal diversity, '
                         'mean nearest-neighbour similarity)')
    ap.add_argument('--fp_radius', type=int, default=None, help=f'radius of the fingerprint, 0 .. {FP_MAX_RADIUS} (default {FP_RADIUS})')
    ap.add_argument('--diverse', type=int, default=None, metavar='K',
                    help='implies --fingerprints: writes <outdir>/<name>_diverse.txt, the MaxMin picks (index, pick_sim) in pick order')
    ap.add_argument('--reference_fps', type=str, default=None, metavar='FILE.npy',
                    help='implies --fingerprints: uint64 [m, 32]; writes <outdir>/<name>_nearest.txt, per finished molecule the nearest '
                         'similarity to that set and the row that attains it')
    ap.add_argument('--substructure', type=str, default=None, metavar='patterns.json',
                    help='implies --valid_only: a molecule whose anchors of a pattern lie outside its min / max is not finished; writes '
                         '<outdir>/<name>_substructure.txt')
    ap.add_argument('--substructure_steps', type=int, default=None, metavar='N',
                    help=f'with --substructure: the work bound per root, 1 .. 2**30 (default {substruct.DEFAULT_STEPS})')
    ap.add_argument('--add_edge', type=str, default='predicted', choices=['predicted', 'distance', 'openbabel'],
                    help="where the bonds come from (the reference driver's spelling): 'predicted' = argmax of the bond scores; 'distance' "
                         "(implies --valid_only) = perceived from the sampled coordinates, every screen and analysis then runs on those "
                         "bonds; 'openbabel' is not supported")
    ap.add_argument('--bond_agreement', action='store_true',
                    help='implies --valid_only: writes <outdir>/<name>_bond_agreement.txt, per finished molecule how the predicted and the '
                         'distance bonds agree, and the .sdf files carry the counts as the data item PHOREGEN_BONDS')
    ap.add_argument('--hydrogens', action='store_true',
                    help='implies --valid_only: places the hydrogens of the Kekulé form in 3D; .sdf blocks are written as all-atom blocks')
    ap.add_argument('--hydrogen_options', type=json.loads, default=None,
                    help='JSON object replacing single options of HydrogenOptions (with --hydrogens): xh_length, clash_min, max_contacts')
    ap.add_argument('--scaffolds', action='store_true',
                    help='implies --valid_only: writes <outdir>/<name>_scaffolds.txt (per finished molecule its Murcko scaffold key, framework '
                         'key, group, sizes and scaffold SMILES) and <name>_scaffold_summary.txt')
    ap.add_argument('--scaffold_plain', action='store_true',
                    help='with --scaffolds: the plain Bemis-Murcko framework, without the atoms double-bonded to a ring or a linker')
    ap.add_argument('--max_per_scaffold', type=int, default=None, metavar='K',
                    help='implies --scaffolds: writes <outdir>/<name>_scaffold_picks.txt, the first K finished molecules of every scaffold')
    ap.add_argument('--properties', action='store_true',
                    help='implies --valid_only: property descriptors of every molecule (weight, tpsa, logp, mr, Lipinski and Veber counts, '
                         'fsp3); writes <outdir>/<name>_properties.txt, the .sdf files carry the data item PHOREGEN_PROPERTIES')
    ap.add_argument('--property_limits', type=json.loads, default=None,
                    help='JSON object (with --properties): {"preset": "lipinski"} or {"preset": "veber"}, or keys of PropertyLimits, e.g. '
                         '{"mol_weight": [null, 450], "sums": {"logp": [null, 4]}, "max_violations": 0}')
    ap.add_argument('--shape', action='store_true',
                    help='implies --valid_only: writes <outdir>/<name>_shape.txt (per finished molecule its volume and its nearest other '
                         'molecule by 3D shape Tanimoto, compared where they lie) and <name>_shape_summary.txt')
    ap.add_argument('--shape_colour', action='store_true',
                    help='with --shape, implies --features: the atoms\' feature types as colour, the score is (1 - W) shape + W colour Tanimoto')
    ap.add_argument('--shape_colour_weight', type=float, default=None, metavar='W', help='with --shape_colour: W in [0, 1] (default 0.5)')
    ap.add_argument('--shape_reference', type=str, default=None, metavar='FILE.sdf',
                    help='implies --shape: the first mol block of the file, in the frame of the .phore file; adds the column '
                         'reference_shape_sim and the summary line mean_reference_shape_similarity')
    ap.add_argument('--shape_align', action='store_true',
                    help='with --shape --shape_reference: the best rigid overlay of the reference onto every finished molecule; adds the '
                         'columns aligned_shape_sim aligned_start (with --shape_colour also aligned_colour_sim aligned_score) and the '
                         'summary line mean_aligned_reference_shape_similarity')
    ap.add_argument('--shape_align_sdf', action='store_true',
                    help='with --shape_align: also writes every finished molecule overlaid onto the reference under <outdir>/sdf_aligned/')
    ap.add_argument('--num_steps', type=int, default=None, help='reverse steps of the sampler (default: the model\'s)')
    ap.add_argument('--sdf', action='store_true', help='write one .sdf per molecule under <outdir>/sdf_results/')
    args = ap.parse_args()
    if args.add_edge == 'openbabel':
        ap.error("--add_edge openbabel is not supported: this project has no OpenBabel; use 'predicted' or 'distance'")
    if args.geom_limits is not None and not args.geometry:
        ap.error('--geom_limits needs --geometry')
    if args.ring_limits is not None and not args.rings:
        ap.error('--ring_limits needs --rings')
    if args.no_charged and not (args.kekule or args.smiles or args.hydrogens):
        ap.error('--no_charged needs --kekule, --smiles or --hydrogens')
    if args.feature_limits is not None and not args.features:
        ap.error('--feature_limits needs --features')
    if args.stereo_limits is not None and not args.stereo:
        ap.error('--stereo_limits needs --stereo')
    if args.hydrogen_options is not None and not args.hydrogens:
        ap.error('--hydrogen_options needs --hydrogens')
    if args.property_limits is not None and not args.properties:
        ap.error('--property_limits needs --properties')
    args.shape = args.shape or args.shape_reference is not None
    if args.shape_colour and not args.shape:
        ap.error('--shape_colour needs --shape')
    if args.shape_colour_weight is not None and not args.shape_colour:
        ap.error('--shape_colour_weight needs --shape_colour')
    shape_weight = 0.5 if args.shape_colour_weight is None else args.shape_colour_weight
    if not 0.0 <= shape_weight <= 1.0:
        ap.error('--shape_colour_weight must lie in [0, 1]')
    args.features = args.features or args.shape_colour
    args.shape_align = args.shape_align or args.shape_align_sdf
    if args.shape_align and args.shape_reference is None:
        ap.error('--shape_align needs --shape --shape_reference FILE')
    shape_reference = None
    if args.shape_reference is not None:
        try:
            shape_reference = first_mol_block_of(open(args.shape_reference).read())
            shape_mod.read_mol_block(shape_reference)
        except (OSError, ValueError) as err:
            ap.error(f'--shape_reference: {err}')
    try:
        property_limits = property_limits_of(args.property_limits) if args.properties else None
    except (ValueError, TypeError) as err:
        ap.error(str(err))
    args.fingerprints = args.fingerprints or args.diverse is not None or args.reference_fps is not None
    if args.fp_radius is not None and not args.fingerprints:
        ap.error('--fp_radius needs --fingerprints')
    fp_radius = FP_RADIUS if args.fp_radius is None else args.fp_radius
    if not 0 <= fp_radius <= FP_MAX_RADIUS:
        ap.error(f'--fp_radius must be 0 .. {FP_MAX_RADIUS}')
    if args.diverse is not None and args.diverse < 0:
        ap.error('--diverse must not be negative')
    reference = None
    if args.reference_fps is not None:
        reference = np.load(args.reference_fps)
        if reference.dtype != np.uint64 or reference.ndim != 2 or reference.shape[1] != FP_WORDS:
            ap.error(f'--reference_fps must hold uint64 [m, {FP_WORDS}], not {reference.dtype} {reference.shape}')
    args.scaffolds = args.scaffolds or args.max_per_scaffold is not None
    if args.scaffold_plain and not args.scaffolds:
        ap.error('--scaffold_plain needs --scaffolds')
    if args.max_per_scaffold is not None and args.max_per_scaffold < 0:
        ap.error('--max_per_scaffold must not be negative')
    if args.substructure_steps is not None and args.substructure is None:
        ap.error('--substructure_steps needs --substructure')
    patterns = None
    if args.substructure is not None:
        steps = substruct.DEFAULT_STEPS if args.substructure_steps is None else args.substructure_steps
        if not 1 <= steps <= substruct.MAX_STEPS:
            ap.error('--substructure_steps must be 1 .. 2**30')
        patterns = (substruct.load_patterns_json(args.substructure), steps)
    args.valid_only = args.valid_only or args.shape or args.scaffolds or args.add_edge != 'predicted' or args.bond_agreement or patterns is not None or args.fingerprints or args.unique or args.geometry or args.rings or args.kekule or args.features or args.smiles or args.stereo or args.hydrogens or args.properties
    stereo_limits = StereoLimits(**(args.stereo_limits or {})) if args.stereo else None
    hydrogen_options = HydrogenOptions(**(args.hydrogen_options or {})) if args.hydrogens else None
    feature_limits = FeatureLimits(**(args.feature_limits or {})) if args.features else None
    geom_limits = GeomLimits(**(args.geom_limits or {}))
    ring_limits = RingLimits(**(args.ring_limits or {})) if args.rings else None
    # (--smiles --no_charged: the text is written from the neutral-only Kekulé form, which the molecules then carry as with --kekule)
    kekule = KekuleOptions(allow_charged=not args.no_charged) if args.kekule or ((args.smiles or args.hydrogens) and args.no_charged) else None
    torch.manual_seed(args.seed)
    cfg = default_model_config()
    if args.config:
        full = load_config(args.config)
        cfg = full.model
        if full.dataset.data_name in ('zinc_300', 'pdbbind'):
            cfg.phore_feat_dim += 2
    model = PhoreDiff(cfg, 'zinc_300')
    if args.check_point:
        model.load_state_dict(torch.load(args.check_point, map_location='cpu')['model'])
    else:
        print('[W] no --check_point: deterministic synthetic weights (molecules will be noise)')
        init_deterministic_(model, 0)
    model = model.eval().to('cuda')
    os.makedirs(args.outdir, exist_ok=True)
    files = json.load(open(args.phore_file_list))
    fragment = load_fragment_json(args.fragment) if args.fragment else None
    for pidx, f in enumerate(files):
        data = parse_phore_file(f).to('cuda')
        done, t0 = [], time.time()
        kw = dict(pos_guidance_opt=args.pos_guidance_opt, sample_mode=args.sample_nodes_mode, normal_scale=args.normal_scale,
                  rng=args.rng, fragment=fragment)
        if args.num_steps is not None:
            kw['num_steps'] = args.num_steps
        if args.valid_only:
            # sample_all.py:79-84,172: top up until num_samples molecules have passed
            geometry = None
            if args.geometry:                                          # the points PhoreDiff.sample reads, in world coordinates
                ph = data['phore']
                geometry = (ph.pos.float() + data.center.float(), ph.x[:, model.ex_col] == 1, geom_limits)
            features = None
            if args.features:                                          # the same points, their kinds by the type columns' names
                ph = data['phore']
                features = (ph.pos.float() + data.center.float(), point_kinds_of(ph.x, PHORETYPES1), feature_limits)
            out = sample_valid(model, data, args.num_samples, batch_size=args.batch_size, unique=args.unique, geometry=geometry,
                               rings=ring_limits, kekule=kekule, features=features, smiles=True if args.smiles else None,
                               stereo=stereo_limits, **(dict(fingerprints=fp_radius) if args.fingerprints else {}),
                               **(dict(substructure=patterns) if patterns is not None else {}),
                               **(dict(add_edge=args.add_edge) if args.add_edge != 'predicted' else {}),
                               **(dict(bond_agreement=True) if args.bond_agreement else {}),
                               **(dict(hydrogens=hydrogen_options) if args.hydrogens else {}),
                               **(dict(properties=property_limits) if args.properties else {}), **kw)
            done = out['finished']
            print(f"Finished {len(done)} | Failed {len(out['failed'])}" + (f" | Duplicates {len(out['duplicates'])}" if args.unique else ''))
            if args.unique:
                with open(os.path.join(args.outdir, data.name + '_keys.txt'), 'w') as fh:
                    fh.writelines('%016x\n' % (m['stereo']['stereo_key'] if args.stereo else m['key']) for m in done)
            if args.bond_agreement:
                with open(os.path.join(args.outdir, data.name + '_bond_agreement.txt'), 'w') as fh:
                    fh.write('# index mode ' + ' '.join(BOND_AGREE_COUNTS) + '\n')
                    fh.writelines('%d %s %s\n' % (i, m['bonds'], ' '.join(str(m['bond_agreement'][k]) for k in BOND_AGREE_COUNTS))
                                  for i, m in enumerate(done))
            if args.smiles:                                            # sample_all.py:157-159
                with open(os.path.join(args.outdir, data.name + '_SMILES_all.txt'), 'w') as fh:
                    fh.writelines(m['smiles']['text'] + '\n' for m in done)
            if patterns is not None:
                with open(os.path.join(args.outdir, data.name + '_substructure.txt'), 'w') as fh:
                    fh.writelines('%d %s %d %d 0x%02x\n' % (i, name, e['embeddings'], e['anchors'], e['status'])
                                  for i, m in enumerate(done) for name, e in m['substructure'].items())
            if args.fingerprints:
                fps = similarity.stack(done, 'cuda')
                np.save(os.path.join(args.outdir, data.name + '_fingerprints.npy'), fps.cpu().numpy().view(np.uint64))
                near = similarity.nearest(fps)
                n = len(done)
                diversity = similarity._diversity(near.sum.sum().item(), n)
                with open(os.path.join(args.outdir, data.name + '_similarity.txt'), 'w') as fh:
                    fh.write('%d %.6f %.6f\n' % (n, diversity, near.sim.double().mean().item() if n >= 2 else float('nan')))
                if args.diverse is not None:
                    picks = similarity.maxmin_pick(fps, min(args.diverse, n))
                    with open(os.path.join(args.outdir, data.name + '_diverse.txt'), 'w') as fh:
                        fh.writelines('%d %.6f\n' % (i, s) for i, s in zip(picks.index.tolist(), picks.sim.tolist()))
                if reference is not None:
                    ref = similarity.nearest(fps, torch.from_numpy(reference.view(np.int64)).to('cuda').contiguous())
                    with open(os.path.join(args.outdir, data.name + '_nearest.txt'), 'w') as fh:
                        fh.writelines('%.6f %d\n' % (s, j) for s, j in zip(ref.sim.tolist(), ref.index.tolist()))
            if args.properties:
                write_property_file(args.outdir, data.name, done)
            if args.shape:
                overlay = write_shape_files(args.outdir, data.name, done, args.shape_colour, shape_weight, shape_reference, args.shape_align)
                if args.shape_align_sdf:
                    aligned_dir = os.path.join(args.outdir, 'sdf_aligned')
                    os.makedirs(aligned_dir, exist_ok=True)
                    moves = zip(overlay.rotation.tolist(), overlay.translation.tolist()) if overlay is not None else ()
                    for i, (m, (rot, shift)) in enumerate(zip(done, moves)):
                        n_h = len(m['hydrogens']['h_parent']) if 'hydrogens' in m else 0
                        if m['status'] & STATUS_NONFINITE or m['bond_type'].numel() + n_h > 999:      # (the rule of sdf_results/ below)
                            continue
                        write_sdf(os.path.join(aligned_dir, f'{pidx}_{data.name}_{i}.sdf'), [overlaid_onto_reference(m, rot, shift)],
                                  names=[f'{data.name}_{i}'])
            if args.scaffolds:
                write_scaffold_files(args.outdir, data.name, done, not args.scaffold_plain, args.max_per_scaffold)
        while len(done) < args.num_samples and not args.valid_only:
            n = min(args.batch_size, args.num_samples - len(done))
            res = model.sample(data, n, 'cuda', return_traj=False, **kw)
            # sample_all.py:104-116 (`.cpu()` of everything, unbatch_data, decode_data) in one pass: argmax on the device,
            # one copy of the compact arrays (with --sdf: the a < b bonds and the screen's verdict with them)
            done += assemble(res) if args.sdf else decode_batch(res, include_bond=True)
        torch.save(done, os.path.join(args.outdir, data.name + '.pt'))
        if args.sdf:
            sdf_dir = os.path.join(args.outdir, 'sdf_results')
            os.makedirs(sdf_dir, exist_ok=True)
            n_sdf = 0
            for i, m in enumerate(done):
                n_h = len(m['hydrogens']['h_parent']) if 'hydrogens' in m else 0         # (an all-atom block has a bond per hydrogen)
                if m['status'] & STATUS_NONFINITE or m['bond_type'].numel() + n_h > 999:      # non-finite coordinates / more bonds than a V2000 block counts
                    continue
                write_sdf(os.path.join(sdf_dir, f'{pidx}_{data.name}_{i}.sdf'), [m], names=[f'{data.name}_{i}'])
                n_sdf += 1
            print(f'{data.name}: {n_sdf} .sdf files in {sdf_dir}')
        print(f'{data.name}: {len(done)} samples in {time.time() - t0:.1f} s')


if __name__ == '__main__':
    main()
