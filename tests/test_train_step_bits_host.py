"""The comparison's own arithmetic of tests/test_gpu_train_step_bits.py, on known answers and without a GPU: the rule by which
tests/golden/make_train_step_bits.py stores a large array (SHA-256 of its bytes plus its first elements), the order in which float
bits are compared (a difference is a distance in ulps), and that the recorded file holds what the generator's lists name."""
import hashlib
import os

import numpy as np

from tests.golden import make_train_step_bits as MK


def test_large_arrays_are_stored_as_sha256_of_their_bytes_and_a_head():
    out = {}
    big = np.arange(MK.FULL + 1, dtype=np.float32)
    MK.record(out, "x", big)
    MK.record(out, "y", big[:MK.FULL])
    assert sorted(out) == ["x.head", "x.sha256", "y"] and out["x.head"].size == MK.HEAD and out["y"].size == MK.FULL
    assert bytes(out["x.sha256"]) == hashlib.sha256(big.tobytes()).digest()


def test_ordered_bits_count_ulps_across_zero():
    a = np.array([-1.0, -np.float32(1e-45), -0.0, 0.0, np.float32(1e-45), 1.0], np.float32)
    o = MK.ordered(a).tolist()
    assert o == sorted(o) and o[2] == o[3] and o[3] - o[1] == 1 and o[4] - o[3] == 1
    one = np.array([1.0], np.float32)
    assert int(MK.ordered(np.nextafter(one, np.float32(2)))[0] - MK.ordered(one)[0]) == 1
    assert int(MK.ordered(np.array([1.0]))[0] - MK.ordered(np.nextafter(np.array([1.0]), 0.0))[0]) == 1


def test_the_recorded_file_holds_the_calls_the_generator_names():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(MK.__file__)), "train_step_bits.npz")) as z:
        keys = set(z.files)
    for name in MK.LOSS_CASES:
        for call in ["default", "default_dev", "default_mixed", "ciou_g2_mixed"] + ["%s_g%g" % o for o in MK.LOSS_OPTIONS]:
            assert "loss/%s/%s/losses" % (name, call) in keys, (name, call)
    for name, _, _, pid in MK.DISTILL_CALLS:
        assert "distill/%s/%s/distill3" % (name, pid) in keys
    assert "optimizer/legacy/sha256" in keys and "optimizer/legacy_unaligned/sha256" in keys and "optimizer/overflow/found_inf" in keys
