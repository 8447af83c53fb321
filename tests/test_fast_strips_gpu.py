"""k_fast_cells' strips against the oracle: the frames of tests/fast_strip_cases.py (tests/test_fast_strips_cpu.py proves what each reaches) through OrbExtractor,
batched by size -- FAST candidates of every level, keypoints and descriptors -- as tests/test_guest_budget_gpu.py compares its mixed batch."""
import numpy as np
import pytest
import fast_strip_cases as fc
from synth import synth_frame, noise_frame

pytestmark = pytest.mark.gpu

BATCHES = {      # frames of one size go through one launch
    "rows_1_K": ["row1"], "rows_K": ["rowK"], "rows_K1": ["rowK1"],
    "w250": ["row2K1", "ini_min", "empty_between"],       # rows of 2K + 1 cells: full strips and a strip of one cell
    "small": ["small"],
    "cap": ["at_cap", "cap_plus_1", "at_cap"],             # the restart path between two frames on the list path
    "noise320": ["noise320"],
    "bands": ["bands"],
}


def _run_batch(fe, ctx, oracle, imgs, nfeat):
    import torch
    h, w = imgs[0].shape
    n = len(imgs)
    ex = fe.OrbExtractor(ctx, nfeat, 1.2, fc.NLEVELS, fc.INI_TH, fc.MIN_TH)
    try:
        cap = nfeat + 64 * fc.NLEVELS
        d = torch.from_numpy(np.stack(imgs)).cuda()
        d_kp = torch.zeros(n * cap * 28, dtype=torch.uint8, device="cuda"); d_desc = torch.zeros(n * cap * 32, dtype=torch.uint8, device="cuda")
        d_n = torch.zeros(n, dtype=torch.int32, device="cuda")
        ex.extract_batch_dev(d, w, h, w, w * h, n, d_kp, d_desc, d_n, cap)
        torch.cuda.synchronize(); ctx.synchronize()
        kp = d_kp.cpu().numpy().view(fe.KP_DTYPE).reshape(n, cap); desc = d_desc.cpu().numpy().reshape(n, cap, 32); cnt = d_n.cpu().numpy()
        total = 0
        for i, img in enumerate(imgs):
            for l in range(fc.NLEVELS):
                np.testing.assert_array_equal(ex.debug_candidates(i, l), oracle.candidates(img, l, nfeat), err_msg="frame %d FAST candidates level %d" % (i, l))
            okp, odesc = oracle.orb_extract(img, nfeat)
            assert cnt[i] == len(okp)
            np.testing.assert_array_equal(kp[i, :cnt[i]].view(np.uint8), okp.view(np.uint8), err_msg="frame %d keypoints" % i)
            np.testing.assert_array_equal(desc[i, :cnt[i]], odesc, err_msg="frame %d descriptors" % i)
            total += len(okp)
        return total
    finally:
        ex.close()


@pytest.mark.parametrize("batch", list(BATCHES))
def test_strip_frames_against_the_oracle(fe, ctx, oracle, batch):
    imgs = [fc.frame(n) for n in BATCHES[batch]]
    assert _run_batch(fe, ctx, oracle, imgs, 1000 if imgs[0].shape[1] >= 640 else 300) > 0


def test_dense_and_sparse_frames_in_one_launch(fe, ctx, oracle):
    """strips that start their list again and strips that do not, in one launch: noise, a synthetic scene, the border bands, noise again"""
    imgs = [noise_frame(7), synth_frame(1234), fc.frame("bands"), noise_frame(8)]
    assert _run_batch(fe, ctx, oracle, imgs, 1000) > 0
