"""The controller of the adaptive augmentation on the GPU (csrc/augment.hip: sp_ada_observe / sp_ada_adjust; ops.AdaptiveAugment;
DESIGN.md section 15) against the numpy restatement of tests/ada_restated.py: EXACT equality of all eight state words after every launch.
Nothing here has a tolerance - the counts are integers, r is one correctly rounded fp32 division of two exactly converted integers and
p one fp32 addition and two selections.

numel in {1, 63, 64, 65, 257, 512, 51200}: below, at and above a wave, the aligned 16-byte path with a scalar tail and above the block (1024 threads), and the size of
D's prediction tensor at batch 20.  The values sit at the threshold and one ulp to either side, with NaN and +-inf among them."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ada_restated as R  # noqa: E402
from semantic_pyramid_for_image_generation_amd import _lib as L  # noqa: E402
from semantic_pyramid_for_image_generation_amd import ops  # noqa: E402

F = np.float32
NUMELS = (1, 63, 64, 65, 257, 512, 51200)
CANARY = 0x5A5A5A5A


def _dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _values(numel, threshold, seed):
    """fp32 values drawn from {threshold, one ulp above, one ulp below, NaN, +inf, -inf, far above, far below}."""
    t = F(threshold)
    pool = np.array([t, np.nextafter(t, F(np.inf)), np.nextafter(t, F(-np.inf)), np.nan, np.inf, -np.inf, t + F(3), t - F(3)], dtype=F)
    rng = np.random.RandomState(seed)
    return pool[rng.randint(0, len(pool), size=numel)]


class _State:
    """8 words of device state between two canary words, driven through the C ABI, with the restated controller beside it."""

    def __init__(self, p):
        self.buf = torch.full((10,), CANARY, dtype=torch.int32, device=_dev())
        self.buf[1:9] = torch.tensor(R.Controller(p).words(), dtype=torch.int32)
        self.ref = R.Controller(p)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + 4)

    def observe(self, x, threshold, misalign=0):
        """misalign: elements by which the values sit behind a 16-byte boundary (the kernel then takes its scalar path)."""
        xd = torch.full((x.size + misalign + 4,), float("inf"), device=self.buf.device)      # +inf around the values: counted if ever read
        xd[misalign:misalign + x.size] = torch.from_numpy(x).to(self.buf.device)
        L.call("sp_ada_observe", ctypes.c_void_p(xd.data_ptr() + 4 * misalign), x.size, float(threshold), self.ptr, ops.stream())
        self.ref.observe(x, threshold)

    def adjust(self, interval, target, step):
        L.call("sp_ada_adjust", self.ptr, interval, float(target), float(step), ops.stream())
        self.ref.adjust(interval, target, step)

    def check(self, what):
        got = self.buf.cpu().tolist()
        assert got[0] == CANARY and got[9] == CANARY, what
        assert got[1:9] == self.ref.words(), (what, got[1:9], self.ref.words())


@pytest.mark.parametrize("numel", NUMELS)
def test_observe_counts_exactly(numel):
    for threshold in (0.5, 0.0, -0.07):
        st = _State(0.25)
        for rep in range(3):                              # the counts ACCUMULATE: a launch adds to the ones before it
            st.observe(_values(numel, threshold, 7 * numel + rep), threshold, misalign=rep)      # 16-byte aligned, then 4 and 8 bytes behind
            st.check((numel, threshold, rep))
    st = _State(0.0)
    st.observe(np.full(numel, np.nan, dtype=F), 0.5)      # nothing but NaN: total only
    assert (st.ref.pos, st.ref.neg, st.ref.total) == (0, 0, numel)
    st.check((numel, "nan"))


@pytest.mark.parametrize("interval", [1, 3])
def test_windows_move_p_as_the_restatement_does(interval):
    """Twelve steps: above the target until p has reached 1 and stayed there, then below it until p has reached 0 and stayed there - both
    clamps - with a step that is no power of two (every p on the way is a rounded fp32 sum)."""
    st = _State(0.0)
    step, target = F(0.3), 0.2
    high = np.array([1, 1, 1, 0, 1], dtype=F)             # r = 3 / 5 > 0.2
    low = np.array([0, 0, 1, 0, 0.5], dtype=F)            # r = -2 / 5 < 0.2 (one value ON the threshold)
    seen = []
    for i in range(12 * interval):
        st.observe(high if i < 6 * interval else low, 0.5)
        st.adjust(interval, target, step)
        st.check((interval, i))
        seen.append(float(st.ref.p))
    assert max(seen) == 1.0 and seen[6 * interval - 1] == 1.0 and seen[-1] == 0.0 and int(st.ref.adjustments) == 12
    assert len(set(seen)) > 4


def test_r_exactly_on_the_target_holds_p_and_an_empty_window_only_restarts_the_count():
    st = _State(0.5)
    st.observe(np.array([1, 1, 1, 0], dtype=F), 0.5)      # r = 2 / 4 = 0.5 exactly
    st.adjust(1, 0.5, 0.25)
    assert st.ref.p == F(0.5) and st.ref.r_last == F(0.5) and st.ref.adjustments == 1
    st.check("r == target")
    st.observe(np.array([1, 0, 0.5, np.nan], dtype=F), 0.5)      # r = 0 / 4 = target 0
    st.adjust(1, 0.0, 0.25)
    assert st.ref.p == F(0.5) and st.ref.r_last == F(0.0)
    st.check("r == 0 == target")
    for i in range(3):                                   # no observation at all: steps runs to the interval and starts again
        st.adjust(2, 0.0, 0.25)
        st.check(("empty", i))
    assert (st.ref.steps, st.ref.adjustments) == (1, 2)
    # r = 1 / 3: the correctly rounded fp32 quotient, and +-1 exactly at the ends
    for values, target in (([1, 1, 0], 1.0 / 3.0), ([1, 1, 1], 1.0), ([0, 0, 0], -1.0)):
        st = _State(0.5)
        st.observe(np.array(values, dtype=F), 0.5)
        st.adjust(1, target, 0.25)
        st.check(values)


def test_refused_arguments_leave_the_state_untouched():
    st = _State(0.25)
    st.observe(_values(65, 0.5, 1), 0.5)
    st.adjust(3, 0.0, 0.25)
    before = st.buf.cpu().tolist()
    lib = L.lib()
    x = torch.zeros(8, device=_dev())
    nan = float("nan")
    for numel in (0, -1, (1 << 24) + 1):
        assert lib.sp_ada_observe(ops.ptr(x), numel, 0.5, st.ptr, ops.stream()) != 0
    assert lib.sp_ada_observe(None, 8, 0.5, st.ptr, ops.stream()) != 0
    for interval, target, step in ((0, 0.0, 0.25), (1, 1.5, 0.25), (1, -1.5, 0.25), (1, nan, 0.25), (1, 0.0, -0.25), (1, 0.0, 1.5), (1, 0.0, nan)):
        assert lib.sp_ada_adjust(st.ptr, interval, target, step, ops.stream()) != 0
    torch.cuda.synchronize()
    assert st.buf.cpu().tolist() == before
    st.check("after the refusals")


def test_adaptive_augment_owns_the_state_and_round_trips_it():
    dev = _dev()
    ada = ops.AdaptiveAugment(dev, p=0.25, target=0.0, interval=2, speed_images=64, threshold=0.5)
    ref = R.Controller(0.25)
    assert ada.step_size(8) == 0.25 and ada.p.data_ptr() == ada.state.data_ptr() and ada.p.dtype == torch.float32
    x = _values(257, 0.5, 3)
    for i in range(3):
        ada.observe(torch.from_numpy(x).to(dev).view(257, 1))
        ada.adjust(8)
        ref.observe(x, 0.5)
        ref.adjust(2, 0.0, 0.25)
    assert ada.state.cpu().tolist() == ref.words()
    v = ada.values()
    assert v["p"] == float(ref.p) and v["r_last"] == float(ref.r_last) and v["steps"] == 1 and v["adjustments"] == 1 and v["total"] == 257
    sd = ada.state_dict()
    other = ops.AdaptiveAugment(dev)
    ptr = other.state.data_ptr()
    other.load_state_dict(sd)
    assert other.state.data_ptr() == ptr and other.state.cpu().tolist() == ref.words()          # in place: a captured graph's pointer holds
    assert other.settings() == ada.settings()
    fixed = ops.AdaptiveAugment(dev, p=0.5, adaptive=False)                                     # a fixed p: never observed, never adjusted
    fixed.observe(torch.ones(4, device=dev))
    fixed.adjust(8)
    assert fixed.state.cpu().tolist() == R.Controller(0.5).words()
    with pytest.raises(L.SempyrError):
        ada.observe(torch.ones(4, device=dev, dtype=torch.float64))
