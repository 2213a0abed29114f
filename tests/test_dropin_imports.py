"""The `dropin/` alias packages: the reference's own import lines must resolve to phoregen_amd with ONE sys.path entry
(SURVEY.md 8(b) "Import surface the callers use").  Runs in a fresh interpreter so that this test session's own `models` /
`utils` imports cannot leak in.  The second test puts a stand-in reference checkout, written at test time, behind the aliases."""
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(code, extra_path=()):
    env = dict(os.environ)
    env.pop('PYTHONPATH', None)
    prog = 'import sys\n' + ''.join(f'sys.path.insert(0, {p!r})\n' for p in reversed([os.path.join(ROOT, 'dropin'), *extra_path])) + \
        textwrap.dedent(code)
    r = subprocess.run([sys.executable, '-c', prog], capture_output=True, text=True, cwd='/tmp', env=env, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_alias_packages_resolve_to_phoregen_amd():
    out = _run('''
        from models.diffusion import PhoreDiff
        from models.model_utils import EMA
        import models
        from models.uni_denoiser import UniTransformerO2TwoUpdateGeneralBond, NodeUpdateLayer
        from models.common import MLP, GaussianSmearing, get_beta_schedule
        from models.transition import ContigousTransition, GeneralCategoricalTransition
        from utils.sample_utils import unbatch_data, decode_data, make_edge_data, sample_from_interval, MolReconsError
        assert PhoreDiff.__module__ == 'phoregen_amd.models.diffusion'
        assert models.get_denoiser_net.__module__ == 'phoregen_amd.models' and callable(models.get_phore_encoder)
        assert unbatch_data.__module__ == 'phoregen_amd.utils.sample_utils'
        from phoregen_amd.config import default_model_config
        m = PhoreDiff(default_model_config(), 'zinc_300')
        assert len(m.state_dict()) == 641 and callable(m.phore_encoder.forward)
        print('ok')
    ''')
    assert out.strip().endswith('ok')


# A stand-in for a reference checkout placed behind the alias packages: the reference's own `models` package (which the alias must
# shadow), `utils/misc.py` and `utils/sample_utils.py` (reference-owned modules the extended `utils` package path must still find),
# and a `run` package.  Written at test time, so the test needs nothing outside the repository.
_STANDIN_CHECKOUT = {
    'models/__init__.py': '',
    'models/diffusion.py': 'class PhoreDiff:  # the alias must win over this one\n    pass\n',
    'models/model_utils.py': 'class EMA:  # the alias must win over this one\n    pass\n',
    'utils/__init__.py': '',
    'utils/misc.py': 'def seed_all(seed):\n    return seed\n',
    'utils/sample_utils.py': 'class MolReconsError(Exception):\n    pass\n\n\ndef reconstruct_from_generated_with_edges(*args, **kwargs):\n'
                             '    raise MolReconsError()\n',
    'run/__init__.py': '',
}


def test_reference_scripts_import_unchanged(tmp_path):
    """A caller's imports resolve with the alias packages first on sys.path and a reference checkout behind them: `models` and
    `utils.sample_utils` are phoregen_amd's, every other `utils.*` module is the checkout's own, and the molecule reconstruction
    (`MolReconsError`, `reconstruct_from_generated_with_edges`) is handed through to the checkout's `utils/sample_utils.py`."""
    checkout = tmp_path / 'reference'
    for rel, text in _STANDIN_CHECKOUT.items():
        (checkout / rel).parent.mkdir(parents=True, exist_ok=True)
        (checkout / rel).write_text(text)
    standins = os.path.join(ROOT, 'oracle', 'standins')       # the third-party wheels this image lacks (test infrastructure)
    out = _run(f'''
        from torch_geometric.loader import DataLoader, DataListLoader
        from torch_geometric.data import Batch
        from utils.misc import *
        from models.diffusion import PhoreDiff
        from utils.sample_utils import unbatch_data, decode_data, reconstruct_from_generated_with_edges, MolReconsError
        assert PhoreDiff.__module__ == 'phoregen_amd.models.diffusion', PhoreDiff.__module__
        assert unbatch_data.__module__ == 'phoregen_amd.utils.sample_utils' and decode_data.__module__ == unbatch_data.__module__
        assert seed_all.__module__ == 'utils.misc' and sys.modules['utils.misc'].__file__.startswith({str(checkout)!r})   # the checkout's own file
        from models.model_utils import EMA
        import run
        assert EMA.__module__ == 'phoregen_amd.models.model_utils'
        assert run.__file__.startswith({str(checkout)!r})
        assert MolReconsError.__module__ in ('utils._reference_sample_utils', 'utils.sample_utils')
        assert reconstruct_from_generated_with_edges.__module__ == 'utils._reference_sample_utils'
        print('ok')
    ''', extra_path=(str(checkout), standins))
    assert out.strip().endswith('ok')
