"""The split-once form of the fused split-bf16 dW (create option dw_stage=split_once, k_dwf_so) against
its LDS-DMA form (dw_stage=dma, k_dwf_bx).

k_dwf_so loads each stage into registers, splits every fp32 value once per workgroup into its three bf16
pieces and stores them into a piece image that the waves read with transposed LDS reads; k_dwf_bx stages
the fp32 rows by LDS DMA and every consuming wave splits its own operands. The pieces, the MFMA sequence,
the chunking and the accumulator layout are the same, so the two forms must agree bitwise: gradient,
stepped parameters and loss statistics of the same minibatch.

Shapes: ragged M = 15 996 (OP = 32, a partly filled last stage), OP = 16 (M = 16 384), M = 6 300 with
O = 11, and M = 7 (one chunk of one partly filled stage: the pipeline's prologue with nothing behind it);
these minibatches run two output slices per chunk, so the ragged shape and an OP = 16 one also run with
dw_slices=1, the geometry of minibatches above 32 768 rows; all nine and eight piece products
(dw_mfma=bf16x9 / bf16x8) on one shape each. The CPU test checks the image's offset map.
"""
import ctypes

import numpy as np
import pytest

import oracle_lib as O

ppo_amd = pytest.importorskip("ppo_amd")
from ppo_amd import DeviceArray  # noqa: E402
from test_gpu_parity import fill_storage, make_agent, random_params  # noqa: E402


def test_piece_image_offset_map_is_a_bijection():
    """ppo_dw_image_offset(row, col) (dwso_off: the byte offset of the four bf16 of columns col .. col + 3
    of a stage row in one piece's 16 x 256 image) maps the 16 x 64 groups one to one onto the 8-byte slots
    of the 8 KB image, so every group is 8-byte aligned and no two overlap; and the four rows x 32 columns
    that a 32-lane half takes in one transposed read are 256 contiguous bytes (each LDS bank pair once)."""
    f = ppo_amd.lib().ppo_dw_image_offset
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int, ctypes.c_int]
    off = np.array([[f(r, c) for c in range(0, 256, 4)] for r in range(16)])
    assert (off % 8 == 0).all()
    assert sorted(off.ravel().tolist()) == list(range(0, 16 * 256 * 2, 8))
    for r0 in range(0, 16, 4):
        for c0 in range(0, 256, 32):
            blk = off[r0:r0 + 4, c0 // 4:c0 // 4 + 8].ravel()
            assert blk.min() % 256 == 0 and sorted(blk.tolist()) == list(range(blk.min(), blk.min() + 256, 8))
    assert f(16, 0) < 0 and f(0, 256) < 0 and f(0, 2) < 0 and f(-1, 0) < 0


@pytest.mark.gpu
@pytest.mark.parametrize("E,T,O_,opts", [(3999, 4, 17, "dw_mfma=bf16x6"), (3999, 4, 17, "dw_mfma=bf16x9"),
                                         (512, 32, 16, "dw_mfma=bf16x6"), (700, 9, 11, "dw_mfma=bf16x6"),
                                         (7, 1, 17, "dw_mfma=bf16x6"),
                                         # one output slice per chunk, the metric minibatch's geometry, at small M
                                         (3999, 4, 17, "dw_mfma=bf16x6,dw_slices=1"),
                                         (512, 8, 16, "dw_mfma=bf16x8,dw_slices=1")])
def test_dw_split_once_is_bitwise_the_dma_form(E, T, O_, opts):
    mfma = opts.split(",")[0].split("=")[1]
    M = E * T
    rng = np.random.default_rng(47)
    A, H = 6, 256
    L = O.layout_init(1, O_, A, H)
    p = random_params(L, rng)
    x = rng.standard_normal((M, O_)).astype(np.float32)
    act = rng.uniform(-0.95, 0.95, (M, A)).astype(np.float32)
    olp = (rng.standard_normal(M) * 0.3 - 3.0).astype(np.float32)
    adv = rng.standard_normal(M).astype(np.float32)
    ret = rng.standard_normal(M).astype(np.float32)
    ov = rng.standard_normal(M).astype(np.float32)
    perm = rng.permutation(M).astype(np.int32)
    out = []
    for stage in ("dma", "split_once"):
        ag = make_agent(1, O_, A, H, E, T=T, MB=1, EP=1, clip=0.2, ent=0.01,
                        options=f"{opts},dw_stage={stage}")
        try:
            dw = [t for t in ag.kernel_info().split() if t.startswith("dw=")][0]
            assert dw == "dw=k_dwf_bx/" + mfma + ("/split_once" if stage == "split_once" else ""), ag.kernel_info()
            ag.load_params(p)
            fill_storage(ag, T, E, x, act, olp, adv, ret, ov)
            st = ag.update(2.5e-4, perms=DeviceArray.from_numpy(perm), want_stats=True)
            out.append((ag.last_grad(), ag.params(), st))
        finally:
            ag.close()
    (g0, p0, s0), (g1, p1, s1) = out
    assert np.isfinite(g0).all() and np.linalg.norm(g0) > 0
    np.testing.assert_array_equal(g1, g0)
    np.testing.assert_array_equal(p1, p0)
    assert s0 == s1


@pytest.mark.gpu
def test_dw_split_once_refused_where_it_does_not_apply():
    with pytest.raises(ppo_amd.PPOError, match="dw_stage=split_once"):
        make_agent(1, 17, 6, 256, 64, options="dw_stage=split_once,h1_handoff=recompute")
    with pytest.raises(ppo_amd.PPOError, match="dw_stage=split_once"):
        make_agent(1, 17, 6, 256, 64, options="dw_stage=split_once,dw_mfma=f32")
