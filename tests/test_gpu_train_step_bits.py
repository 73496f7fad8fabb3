"""The loss, distillation and optimizer entry points against RECORDED bits (tests/golden/train_step_bits.npz).

The other tests of these kernels compare paths with each other and with float64 restatements: the reference loss and the loss with
options, sqdet_optimizer_step and sqdet_optimizer_step_opt share their arithmetic (csrc/loss.hip, csrc/optim.hip), and a change that
moved both would pass them all.  Here every call of tests/golden/make_train_step_bits.py is made again and compared bit for bit --
integer views, np.array_equal; large arrays by the SHA-256 of their bytes and their first elements -- with what the same call gave
when the file was written.

The file was recorded on an MI355X with the library built from commit 8ad37630 ("Add knowledge distillation: a teacher net's
ConvDet output in the loss"), the last one BEFORE the loss and optimizer kernels were folded into one body per pass (loss_kernel /
loss_opt_kernel, opt_*_kernel / opt_*_opt_kernel as two copies each), so it holds that commit's bits.  A ROCm
upgrade that changes expf / logf / powf / atanf changes them legitimately: once the accuracy tests (test_gpu_loss_options.py,
test_gpu_distill.py, test_gpu_train_kernels.py, test_gpu_optimizer_options.py) pass on the new stack, regenerate the file with
tests/golden/make_train_step_bits.py.  (tests/test_train_step_bits_host.py checks the digest rule and the ulp order without a GPU.)
"""
import os

import numpy as np
import pytest

from tests.golden import make_train_step_bits as MK

pytestmark = pytest.mark.gpu
_GOLDEN = {}


def golden(prefix):
    if not _GOLDEN:
        with np.load(os.path.join(os.path.dirname(os.path.abspath(MK.__file__)), "train_step_bits.npz")) as z:
            _GOLDEN.update({k: z[k] for k in z.files})
    return {k: v for k, v in _GOLDEN.items() if k.startswith(prefix)}


def check(got, prefix):
    want = golden(prefix)
    assert want and sorted(got) == sorted(want), "the calls made are not the calls recorded: %s" % sorted(set(got) ^ set(want))
    failures = []
    for key in sorted(want):
        g, w = got[key], want[key]
        assert g.dtype == w.dtype and g.shape == w.shape, key
        if g.dtype.kind != "f":
            if not np.array_equal(g, w):
                failures.append("%s: %s" % (key, "a digest differs" if key.endswith("sha256") else "%r != %r" % (g.tolist(), w.tolist())))
            continue
        go, wo = MK.ordered(g), MK.ordered(w)
        if not np.array_equal(go, wo):
            d = np.abs(go - wo)
            at = int(d.argmax())
            failures.append("%s: %d of %d elements differ, the largest distance %d ulp at %d (%r, recorded %r)"
                            % (key, int((d != 0).sum()), d.size, int(d.max()), at, g.reshape(-1)[at], w.reshape(-1)[at]))
    print("BITS %s: %d arrays, %d differ" % (prefix, len(want), len(failures)))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", MK.LOSS_CASES)
def test_loss_calls_give_the_recorded_bits(name):
    check(MK.loss_bits(name), "loss/%s/" % name)


def test_distill_calls_give_the_recorded_bits():
    check(MK.distill_bits(), "distill/")


def test_optimizer_steps_give_the_recorded_bits():
    check(MK.optimizer_bits(), "optimizer/")
