"""The comparison every other bit-for-bit test rests on: tests/model_common.py same_bits (and the np.ascontiguousarray spelling
tests/test_oracle_vs_reference.py keeps) and tests/app_checks.py assert_same."""
import numpy as np
import pytest

from tests.app_checks import assert_same
from tests.model_common import same_bits
from tests.test_oracle_vs_reference import same_bits as same_bits_contiguous

SPELLINGS = pytest.mark.parametrize("same", [same_bits, same_bits_contiguous], ids=["asarray", "ascontiguousarray"])


def bits(*words):
    return np.array(words, dtype=np.uint32).view(np.float32)


@SPELLINGS
def test_identical_bits_are_the_same(same):
    a = bits(0, 0x80000000, 1, 0x3f800000, 0x7f7fffff, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc12345)   # zeros, a denormal, inf, NaNs
    assert same(a, a.copy()).all()
    assert same(a.reshape(3, 3), a.reshape(3, 3).copy()).shape == (3, 3)


@SPELLINGS
def test_any_nan_equals_any_nan(same):
    nans = bits(0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0xffc12345)   # quiet, signalling, payloads, both signs
    assert np.isnan(nans).all()
    assert same(nans[:, None], nans[None, :]).all()
    assert not same(nans, bits(0x7f800000)).any() and not same(nans, np.float32(0)).any()


@SPELLINGS
def test_zeros_of_either_sign_differ(same):
    assert np.float32(0.0) == np.float32(-0.0)
    assert not same(bits(0), bits(0x80000000)).any()


@SPELLINGS
def test_one_ulp_apart_differs(same):
    a = np.array([1.0, -1.0, 1e-45, 3e38, 0.1], dtype=np.float32)
    for b in (np.nextafter(a, np.float32(np.inf)), np.nextafter(a, np.float32(-np.inf))):
        assert not same(a, b).any()


def test_assert_same_raises_on_a_shape_mismatch():
    a = np.zeros((2, 3, 4), dtype=np.float32)
    assert_same(a, a.copy(), "equal")
    with pytest.raises(AssertionError):
        assert_same(a.reshape(3, 2, 4), a, "shape")
    with pytest.raises(AssertionError):
        assert_same(a[..., :3], a, "channels")


def test_assert_same_names_the_one_differing_channel():
    want = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    got = want.copy()
    got[1, 2, 3] = np.nextafter(got[1, 2, 3], np.float32(np.inf))
    with pytest.raises(AssertionError) as e:
        assert_same(got, want, "one channel")
    assert "one channel: 1 differing channels" in str(e.value) and "[[1, 2, 3]]" in str(e.value)


def test_assert_same_takes_a_tensor_like():
    class OnDevice:
        def __init__(self, a):
            self.a = a

        def cpu(self):
            return self

        def numpy(self):
            return self.a

    want = bits(0x7fc00000, 0x80000000, 0x3f800000).reshape(1, 3)
    assert_same(OnDevice(want.copy()), want, "tensor-like")
    with pytest.raises(AssertionError):
        assert_same(OnDevice(bits(0x7fc00000, 0, 0x3f800000).reshape(1, 3)), want, "tensor-like, -0 against +0")
