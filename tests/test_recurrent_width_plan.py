"""Host side of the GRU / LSTM width support (no GPU): the size of the packed recurrent-kernel image against a NumPy / torch
restatement of its layout, the width -> C entry routing of the binding, and the refusals that need no device."""
import ctypes

import numpy as np
import pytest
import torch

from gnn_uds_amd import _lib


def frag_k(t, qd, jj):
    """k index of element jj of lane quarter qd in k-step t (kernels_fused.hpp: frag_k)."""
    return 32 * t + (4 * qd + jj if jj < 4 else 16 + 4 * qd + jj - 4)


def reference_pack(U, G):
    """The image uds_recurrent_pack_bwd writes for U (H, G*H), as int16 bf16 bit patterns of shape
    (2G slices, KT k-steps, MB blocks, hi / lo, 64 lanes, 8): slice g = U[:, gH:(g+1)H], slice G + g its transpose;
    element = W[frag_k(t, lane >> 4, jj)][16 m + (lane & 15)], rows from H up zero; hi = bf16(w), lo = bf16(w - hi)."""
    H = U.shape[0]
    MB, KT = H // 16, (H + 31) // 32
    out = torch.zeros(2 * G, KT, MB, 2, 64, 8, dtype=torch.int16)
    k = torch.tensor([[[frag_k(t, lane >> 4, jj) for jj in range(8)] for lane in range(64)] for t in range(KT)])      # (KT, 64, 8)
    for s in range(2 * G):
        g = s % G
        W = U[:, g * H:(g + 1) * H].float()
        W = W if s < G else W.t()
        Wp = torch.zeros(32 * KT, H)
        Wp[:H] = W
        for m in range(MB):
            f = 16 * m + (torch.arange(64) & 15)                                 # (64,)
            w = Wp[k, f[None, :, None].expand(KT, 64, 8)]                        # (KT, 64, 8)
            hi = w.bfloat16()
            lo = (w - hi.float()).bfloat16()
            out[s, :, m, 0] = hi.view(torch.int16)
            out[s, :, m, 1] = lo.view(torch.int16)
    return out


@pytest.mark.parametrize('G', [3, 4])
@pytest.mark.parametrize('H', _lib.RECURRENT_TRAIN_WIDTHS)
def test_packed_size_is_the_layouts(G, H):
    U = torch.randn(H, G * H, generator=torch.Generator().manual_seed(H))
    img = reference_pack(U, G)
    assert img.numel() * 2 == _lib.recurrent_bwd_packed_bytes(H, G)
    assert _lib.load().uds_recurrent_bwd_packed_bytes(H, G - 3) == _lib.recurrent_bwd_packed_bytes(H, G)
    # rows of the K dimension beyond H are zero: lanes of the last k-step whose k index is >= H
    KT = (H + 31) // 32
    if H % 32:
        for lane in range(64):
            for jj in range(8):
                if frag_k(KT - 1, lane >> 4, jj) >= H:
                    assert not img[:, KT - 1, :, :, lane, jj].any()
    # hi + lo restores the weight to 2^-16 relative (what the three-product scheme rests on)
    hi, lo = img[0, 0, 0, 0].view(torch.bfloat16).float(), img[0, 0, 0, 1].view(torch.bfloat16).float()
    w = torch.stack([torch.stack([U[frag_k(0, lane >> 4, jj), lane & 15] if frag_k(0, lane >> 4, jj) < H else torch.tensor(0.)
                                  for jj in range(8)]) for lane in range(64)])
    assert float((hi + lo - w).abs().max()) <= 2.0 ** -16 * float(w.abs().max())


def test_packed_size_at_64_is_the_image_the_old_entry_takes():
    lib = _lib.load()
    for G in (3, 4):
        assert _lib.recurrent_bwd_packed_bytes(64, G) == 2 * G * lib.uds_rowgemm_packed_bytes(64, 64) == 2 * G * 16384


def test_unsupported_widths_have_no_image():
    lib = _lib.load()
    for H in (0, 8, 24, 100, 144, 256, -16):
        assert _lib.recurrent_bwd_packed_bytes(H, 3) == 0 and lib.uds_recurrent_bwd_packed_bytes(H, 0) == 0
        assert _lib.recurrent_bwd_route(H) is None
    assert lib.uds_recurrent_bwd_packed_bytes(64, 2) == 0 and _lib.recurrent_bwd_packed_bytes(64, 5) == 0


def test_width_routing():
    assert _lib.RECURRENT_TRAIN_WIDTHS == (16, 32, 48, 64, 80, 96, 112, 128)
    assert _lib.recurrent_bwd_route(64) == 'uds_recurrent_backward'
    for H in _lib.RECURRENT_TRAIN_WIDTHS:
        if H != 64:
            assert _lib.recurrent_bwd_route(H) == 'uds_recurrent_backward_h'
    for name in ('uds_recurrent_backward', 'uds_recurrent_backward_h', 'uds_recurrent_pack_bwd', 'uds_recurrent_bwd_packed_bytes'):
        assert name in _lib.SYMBOLS and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)


def test_argument_errors_need_no_device():
    lib = _lib.load()
    assert lib.uds_recurrent_backward_h(None, None, None, None, None, None, 1, 1, 1, 32, 0, None, None, None) == -22
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data - buf.ctypes.data % 16 + 16
    assert lib.uds_recurrent_backward_h(p, p, None, p, None, p, 1, 1, 1, 24, 0, p, p, None) == -22 and b'24 units' in lib.uds_last_error()
    assert lib.uds_recurrent_backward_h(p, p, None, p, None, p, 1, 1, 1, 32, 1, p, p, None) == -22 and b'cell states' in lib.uds_last_error()
    assert lib.uds_recurrent_pack_bwd(p, 40, 0, p, None) == -22
    with pytest.raises(_lib.UdsError, match='recurrent_pack_bwd'):
        _lib.recurrent_pack_bwd(torch.zeros(24, 72))
    with pytest.raises(_lib.UdsError, match='recurrent_pack_bwd'):
        _lib.recurrent_pack_bwd(torch.zeros(32, 64))


def test_layer_refuses_other_widths_under_gradients_before_touching_the_device():
    from gnn_uds_amd.emulator import GRU, LSTM
    for cls in (GRU, LSTM):
        mod = cls(24, in_features=8, generator=torch.Generator().manual_seed(0))
        mod.requires_grad_(True)
        with pytest.raises(NotImplementedError, match=r'16, 32, 48, 64, 80, 96, 112, 128'):
            mod(torch.zeros(1, 2, 3, 8))
