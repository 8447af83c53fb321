"""GPU: the library takes the forms csrc/lines_form.h decides.  tests/test_lines_form_cpu.py checks the rule itself on a stand-alone dump of the header
(tests/sim/lines_form_dump.cpp); here sslam_lines_extract_batch_dev runs small calls on both sides of the frame-count boundaries a handful of frames reach, and what
sslam_testing_lines_last_forms reports must be the dump's row for the same sizes, knobs and the device's compute-unit count.  160 x 120 is the smallest frame the fused
gradient kernel takes.  The large-batch rows are tests/test_lsd_forms_gpu.py's."""
import numpy as np
import pytest
import torch
import lsd_cases as lc
import plan_dump
from test_lines_form_cpu import FIELDS, _row

pytestmark = pytest.mark.gpu

W, H, SW, SH = 160, 120, 128, 96
MAX_LINES, CAP = 40, 64
KNOBS = ("SSLAM_NFA_STREAM", "SSLAM_NFA_FUSED", "SSLAM_LSD_FLAVOUR", "SSLAM_LSD_PERSIST", "SSLAM_LSD_CLUSTER", "SSLAM_CL_WGS", "SSLAM_CL_WINDOW", "SSLAM_CL_NO_FEEDER",
         "SSLAM_CL_SMAP", "SSLAM_NFA_STREAM_TICKS")


@pytest.mark.parametrize("knobs", [{}, {"SSLAM_NFA_STREAM": "0"}], ids=["default", "stream0"])
@pytest.mark.parametrize("nframes", [1, 16, 64, 65])
def test_last_forms_are_the_dumps_row(fe, ctx, monkeypatch, nframes, knobs):
    for k in KNOBS: monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items(): monkeypatch.setenv(k, v)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    line = "forms %d %d %d %d %d %d 0 0" % (W, H, SW, SH, nframes, cus) + "".join(" %s=%s" % kv for kv in knobs.items())
    want = _row(plan_dump.asker(src=plan_dump.LINES_FORM)([line])[0], FIELDS)
    assert want["core"] == ("lone" if nframes == 65 else "cluster" if knobs else "cluster_stream"), want          # (the calls do straddle the boundary at 64 frames)
    frames = torch.from_numpy(lc.strokes(W, H).copy()).cuda()[None].repeat(nframes, 1, 1).contiguous()
    d_kl = torch.zeros(nframes * CAP * 68, dtype=torch.uint8, device="cuda"); d_ld = torch.zeros(nframes * CAP * 32, dtype=torch.uint8, device="cuda")
    d_fn = torch.zeros(nframes * CAP * 3, dtype=torch.float64, device="cuda"); d_n = torch.zeros(nframes, dtype=torch.int32, device="cuda")
    ex = fe.LineExtractor(ctx, MAX_LINES)
    try:
        ex.extract_batch_dev(frames, W, H, W, W * H, nframes, d_kl, d_ld, d_fn, d_n, CAP)
        torch.cuda.synchronize(); ex.ctx.synchronize()
        assert ex.batch_status(CAP) == (0, 0, 0, -1)
        cnt = d_n.cpu().numpy()
        assert cnt[0] > 0 and (cnt == cnt[0]).all(), cnt          # the call did its work: every copy of the frame yields the same lines
        got = ex.last_forms()
        assert got == dict(core=want["core"], grid=want["grid"] if want["core"] == "guest" else 0, fused_grad=True, sort_runs=bool(want["sort_runs"]),
                           nfa="all" if want["nfa"] == "topn" else want["nfa"], eval_waves=want["eval_waves"], count_waves=want["count_waves"],
                           lbd_rpi=want["lbd_rpi"]), (got, want)
    finally:
        ex.close()
