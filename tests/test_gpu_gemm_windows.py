"""Row windows of the streaming GEMM (PgGemm.tile_rows, csrc/gemm_stream.hip): a launch over a list of 64-row windows computes every row a
window covers from its own X row into its own Y row with the bits of the full-row launch of the same form, and touches no other row.
Window lists: one window at the start, one anchored at the end (200 - 64), two that overlap, and five in no order with overlaps."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

M = 200
WINDOW_LISTS = [[0], [136], [10, 40], [0, 136, 70, 3, 64]]
OK, ERR_ARG = 0, 1


def _lib():
    from phoregen_amd import hip
    return hip, hip.lib(), hip.stream_ptr()


@pytest.fixture(scope='module')
def operands():
    g = torch.Generator().manual_seed(11)
    r = lambda *s: torch.randn(*s, generator=g).cuda()
    return dict(X=r(M, 128), W=r(640, 128) / 11.3, bias=r(640), gamma=1.0 + 0.1 * r(128), beta=0.1 * r(128), add=r(M, 640),
                X2=r(M, 20), W148=r(128, 148) / 12.2)


def _gemm(o, N, bias, ln, windows=None, extent=M, W=None, **extra):
    """One launch into a NaN-filled [M, N] buffer.  Returns (status, buffer)."""
    hip, lib, s = _lib()
    Y = torch.full((M, N), float('nan'), device='cuda')
    W = o['W'] if W is None else W
    g = hip.PgGemm()
    g.X, g.ldx, g.K1 = o['X'].data_ptr(), 128, 128
    g.W, g.ldw = W.data_ptr(), W.stride(0)
    g.bias = o['bias'].data_ptr() if bias else None
    if ln:
        g.ln_gamma, g.ln_beta = o['gamma'].data_ptr(), o['beta'].data_ptr()
    g.out_scale = 0.3535533845424652 if ln else 1.0
    g.Y, g.ldy, g.M, g.N = Y.data_ptr(), N, M, N
    keep = [Y, W]
    if windows is not None:
        keep.append(windows)
        g.tile_rows, g.row_extent, g.M = windows.data_ptr(), extent, 64 * windows.numel()
    for k, v in extra.items():
        setattr(g, k, v.data_ptr() if torch.is_tensor(v) else v)
    rc = lib.pg_gemm(C.byref(g), s)
    torch.cuda.synchronize()
    return rc, Y


FORMS = [(128, False, False), (128, True, False), (256, False, False), (256, True, False), (640, False, False), (640, True, False),
         (128, True, True)]


@pytest.fixture(scope='module')
def full_rows(operands):
    """The full-row launch of every form, computed once."""
    out = {}
    for N, bias, ln in FORMS:
        rc, Y = _gemm(operands, N, bias, ln)
        assert rc == OK and bool(torch.isfinite(Y).all())
        out[N, bias, ln] = Y
    return out


@pytest.mark.parametrize('N,bias,ln', FORMS, ids=lambda v: str(v))
@pytest.mark.parametrize('wins', WINDOW_LISTS, ids=lambda w: '-'.join(map(str, w)))
@pytest.mark.parametrize('pinned', [False, True], ids=['device_list', 'pinned_list'])
def test_windows_write_their_rows_with_the_bits_of_the_full_launch(operands, full_rows, N, bias, ln, wins, pinned):
    hip, lib, s = _lib()
    t = torch.tensor(wins, dtype=torch.int32)
    t = t.pin_memory() if pinned else t.cuda()
    rc, Y = _gemm(operands, N, bias, ln, windows=t)
    assert rc == OK, lib.pg_last_error()
    covered = torch.zeros(M, dtype=torch.bool)
    for w0 in wins:
        covered[w0:w0 + 64] = True
    covered = covered.cuda()
    assert torch.equal(Y[covered], full_rows[N, bias, ln][covered])
    assert bool(torch.isnan(Y[~covered]).all())


def test_windows_on_other_forms_are_errors_that_write_nothing(operands):
    hip, lib, s = _lib()
    o = operands
    dev = torch.tensor([0, 136], dtype=torch.int32).cuda()
    cases = [
        dict(windows=dev, add1=o['add'], ld_add1=640),                                      # an added operand (rows add1[r])
        dict(windows=dev, add1=o['add'], ld_add1=640, idx1=torch.arange(M, dtype=torch.int32).cuda(), add_rows=M),
        dict(windows=dev, X2=o['X2'], ldx2=20, K2=20, W=o['W148']),                       # [X | X2]
        dict(windows=dev, act=2),                                                           # not a streaming form
        dict(windows=torch.tensor([0, 137], dtype=torch.int32).pin_memory()),               # beyond extent - 64
        dict(windows=torch.tensor([-1], dtype=torch.int32).pin_memory()),
        dict(windows=torch.tensor([0, 72], dtype=torch.int32).pin_memory(), extent=135),    # ... of a smaller extent
        dict(windows=dev, extent=63),
    ]
    for kw in cases:
        rc, Y = _gemm(o, 128, True, False, **kw)
        assert rc == ERR_ARG and lib.pg_last_error().startswith(b'pg_gemm:'), (kw.keys(), rc, lib.pg_last_error())
        assert bool(torch.isnan(Y).all())


def test_windows_stay_on_the_streaming_kernel_when_the_test_hook_selects_the_tiled_one(operands, full_rows):
    """pg_debug_gemm_streaming(0) moves every other product to the tiled kernel; a windowed product has no tiled form and is not moved."""
    hip, lib, s = _lib()
    dev = torch.tensor([0, 136], dtype=torch.int32).cuda()
    old = lib.pg_debug_gemm_streaming(0)
    try:
        rc, Y = _gemm(operands, 128, True, False, windows=dev)
    finally:
        lib.pg_debug_gemm_streaming(old)
    assert rc == OK, lib.pg_last_error()
    rows = torch.cat([torch.arange(0, 64), torch.arange(136, 200)]).cuda()
    assert torch.equal(Y[rows], full_rows[128, True, False][rows]) and bool(torch.isnan(Y[64:136]).all())
