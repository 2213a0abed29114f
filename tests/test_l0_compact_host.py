"""Layer 0's composed bond-row weights (packing.l0_compose, the sampler pack): W16 = [W[:, :118] @ W_edge | W[:, 118:128]] against a
float64 evaluation of the uncomposed expression, on the three weight profiles of the packing tests.

Bound.  The composed entry is computed in float64 (118 products: relative error below 118 * 2^-53 of sum_j |W[c,j]| |W_edge[j,k]|,
negligible) and rounded ONCE to fp32: |W16[c,k] - exact| <= 2^-24 |exact| <= 2^-24 sum_j |W[c,j]| |W_edge[j,k]|.  The bound below is
that figure with the float64 term added (2^-24 + 2^-45).  Columns that are copied (time smearing, bond-length smearing) are exact."""
import pytest
import torch

from phoregen_amd import packing
from phoregen_amd.config import default_model_config
from phoregen_amd.models.diffusion import PhoreDiff
from phoregen_amd.weights import init_deterministic_

U24 = 2.0 ** -24


@pytest.mark.parametrize('profile', ['default', 'gamma_signed', 'trained_like'])
def test_composed_weights_against_float64(profile):
    m = init_deterministic_(PhoreDiff(default_model_config(), 'zinc_300'), 0, profile=profile).eval()
    pk = packing.ModelPack(m.state_dict(), 6)
    L0, We = pk.layers[0], pk.W_edge_emb.double()
    assert We.shape == (118, 6)
    for name, W, Wc, N, K in (('NB.W_hb', L0.NB.W_hb, L0.NB.W_hb16, 256, 16), ('TB.W_q_hb', L0.TB.W_q_hb, L0.TB.W_q_hb16, 128, 16),
                              ('TB.W_hbg', L0.TB.W_hbg, L0.TB.W_hbg36, 256, 36)):
        assert Wc.shape == (N, K) and Wc.dtype == torch.float32 and Wc.is_contiguous(), name
        W = W.double()
        exact = W[:, :118] @ We
        mag = W[:, :118].abs() @ We.abs()
        err = (Wc[:, :6].double() - exact).abs()
        bound = (U24 + 2.0 ** -45) * mag
        ratio = float((err / bound.clamp_min(1e-300)).max())
        print(f'l0_compose {profile:13s} {name:10s} largest error {float(err.max()):.3e}, largest error / bound {ratio:.3f}')
        assert bool((err <= bound).all()), (profile, name, ratio)
        assert torch.equal(Wc[:, 6:16].double(), W[:, 118:128]), name               # the smearing columns are copies
        if K == 36:
            assert torch.equal(Wc[:, 16:].double(), W[:, 128:148]), name
    # the later layers and the training pack carry no composed weights
    assert not hasattr(pk.layers[1].NB, 'W_hb16')
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    assert not hasattr(packing.ModelPack(sd, 6, detach=False).layers[0].NB, 'W_hb16')


def test_composed_product_equals_the_uncomposed_one_in_float64():
    """[h_edge | ts] . W16^T == h_bond0 . W^T for soft (not one-hot) rows: the identity the engine relies on, in float64."""
    g = torch.Generator().manual_seed(3)
    W, We = torch.randn(128, 128, generator=g).double(), torch.randn(118, 6, generator=g).double()
    h, ts = torch.softmax(torch.randn(40, 6, generator=g), -1).double(), torch.rand(40, 10, generator=g).double()
    hb0 = torch.cat([h @ We.T, ts], 1)
    W16 = packing.l0_compose(W, We)
    assert W16.dtype == torch.float64
    assert torch.allclose(torch.cat([h, ts], 1) @ W16.T, hb0 @ W.T, rtol=0, atol=1e-12)
