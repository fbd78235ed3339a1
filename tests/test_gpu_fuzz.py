"""GPU (-m gpu): a short, seeded slice of tools/fuzz_parity.py -- the public calls against the oracle on random sensor sizes,
event counts around the boundaries of the one-pass paths, hot pixels, every kind of polarity / time-stamp column, every
EVK_IMPL, error semantics; and the event filters, event augmentation, dataset windows / RobustNorm and rotation / xyztheta
warps against the CPU suite's restatements (profiles/fuzz_new_kinds.txt); and the angular-velocity / planar-flow warps
(motion8) and the average-timestamp objective (zhu) against tests/_motion_models8_np.py and tests/_zhu_np.py
(profiles/fuzz_motion8_zhu.txt; what the generators of these two cover is asserted on the CPU by
tests/test_cpu_fuzz_inputs.py over the same seeds); and the five feature sets on the per-pixel grouping -- denoise, tsurf,
corners, planeflow, reconstruct -- against tests/_denoise_np.py, _time_surface_np.py, _corners_np.py, _plane_flow_np.py and
_reconstruct_np.py on one shared stream generator, by the rules of their dedicated GPU tests
(profiles/fuzz_grouping_kinds.txt; coverage asserted by tests/test_cpu_fuzz_inputs.py as well); and the two features that are
defined bit for bit -- emvs (multi-view stereo: votes, packet times, depth map) against tests/_emvs_np.py and simulate (the event
simulator) against tests/_simulate_np.py, every comparison exact (profiles/fuzz_emvs_simulate.txt; coverage asserted by
tests/test_cpu_fuzz_inputs.py over the same seeds); and the kernels that return gradients -- flowts and flowcm (the
average-timestamp and the contrast loss of a dense flow field) against tests/_flow_loss_np.py and tests/_flow_contrast_np.py, segment
(cluster images, loss and gradient, assignment step) against tests/_segmentation_np.py, by the rules and tolerances of
tests/test_gpu_flow_loss.py, test_gpu_flow_contrast.py and test_gpu_segmentation.py, and bit for bit across repeats, forms of input,
batches, directions, autograd and the direct splat (profiles/fuzz_flow_segment.txt, which also holds the three kernel mutations
these slices report; coverage asserted by tests/test_cpu_fuzz_inputs.py over the same seeds); and raw -- the EVT3 / EVT2
decoder against tests/_raw_np.py, bit for bit through the staged and the direct write: the whole stream, its pieces with the state
carried, the out-of-range policies, files in pieces, the encoders' round trip (profiles/fuzz_raw.txt, with the kernel mutations the
slice reports; coverage asserted by tests/test_cpu_fuzz_inputs.py over the same seeds).  (The long runs are recorded in
profiles/r04_fuzz_parity.txt; what they found is pinned by dedicated tests: test_deterministic_mode_at_small_event_counts_views_and_constant_time_stamps,
test_rms_objective_of_a_handful_of_events, the float64 image in test_f11_gather_contrast_and_timestamp_images; the long emvs run of
profiles/fuzz_emvs_simulate.txt: test_dsi_votes_takes_the_table_of_the_callers_poses (tests/test_cpu_emvs.py) and
test_planes_exactly_on_camera_centres_with_unnormalised_quaternions.)"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


@pytest.mark.parametrize("kind,seed0,cases", [("voxel", 100, 60), ("image", 200, 60), ("native", 300, 30), ("iwe", 400, 40),
                                              ("objective", 500, 40), ("windows", 600, 40), ("misc", 700, 60),
                                              ("errors", 800, 80), ("prims", 900, 60), ("search", 1000, 8),
                                              ("filters", 1100, 400), ("augment", 1200, 400), ("datasets", 1300, 300),
                                              ("motion", 1400, 200), ("motion8", 1600, 100), ("zhu", 1800, 80),
                                              ("denoise", 2000, 200), ("tsurf", 2200, 150), ("corners", 2400, 200),
                                              ("planeflow", 2600, 200), ("reconstruct", 2800, 200),
                                              ("emvs", 3040, 150), ("simulate", 3300, 250),
                                              ("flowts", 3700, 150), ("flowcm", 4000, 150), ("segment", 5000, 100),
                                              ("raw", 5100, 200)])
def test_random_cases_agree_with_the_oracle(kind, seed0, cases):
    argv, sys.argv = sys.argv, sys.argv[:1]
    try:
        import fuzz_parity as F
    finally:
        sys.argv = argv
    fn = {"voxel": F.case_voxel, "image": F.case_image, "native": F.case_native, "iwe": F.case_iwe, "objective": F.case_objective,
          "windows": F.case_windows, "misc": F.case_misc, "errors": F.case_errors, "prims": F.case_prims,
          "search": F.case_search, "filters": F.case_filters, "augment": F.case_augment, "datasets": F.case_datasets,
          "motion": F.case_motion, "motion8": F.case_motion8, "zhu": F.case_zhu, "denoise": F.case_denoise, "tsurf": F.case_tsurf,
          "corners": F.case_corners, "planeflow": F.case_planeflow, "reconstruct": F.case_reconstruct, "emvs": F.case_emvs,
          "simulate": F.case_simulate, "flowts": F.case_flowts, "flowcm": F.case_flowcm, "segment": F.case_segment, "raw": F.case_raw}[kind]
    failed = []
    for seed in range(seed0, seed0 + cases):
        desc, err = fn(np.random.default_rng(910_000 + seed))
        if err is not None:
            failed.append("seed %d: %s -> %s" % (seed, desc, err))
    assert not failed, "\n".join(failed)
