"""CPU: oracle/numerics.py -- round_half equals torch's own rounding where torch rounds once, the checker passes correctly
rounded outputs and flags (and locates) each kind of kernel fault the GPU tests are meant to catch."""
import re

import pytest
import torch

from oracle import numerics as nm

HALF = [torch.bfloat16, torch.float16]


def _from_f32(x32, dtype):
    """torch's conversion from float32 (one rounding step, RNE) as float64"""
    return x32.to(dtype).double()


@pytest.mark.parametrize("dtype", HALF)
def test_round_half_equals_torch_on_ties_overflow_and_subnormals(dtype):
    p, emin, vmax = {torch.bfloat16: (8, -126, 3.3895313892515355e38), torch.float16: (11, -14, 65504.0)}[dtype]
    g = torch.Generator().manual_seed(0)
    # exact ties: odd multiples of half an ulp, several binades and both signs
    e = torch.randint(-8, 9, (4096,), generator=g).double()
    m = torch.randint(2 ** (p - 1), 2 ** p, (4096,), generator=g).double()
    ties = (m + 0.5) * torch.exp2(e - (p - 1)) * torch.where(torch.rand(4096, generator=g) < 0.5, -1.0, 1.0).double()
    x = torch.cat([ties, torch.randn(4096, generator=g).double() * 1000, torch.randn(4096, generator=g).double() * 1e-3])
    if dtype == torch.float16:
        # overflow edge: 65504 is the largest finite value, 65520 = 65504 + ulp/2 is the tie that rounds to inf
        x = torch.cat([x, torch.tensor([65504.0, 65519.0, 65519.99, 65520.0, 65536.0, -65520.0, -65519.0, 70000.0])])
        # subnormals (gradual underflow): spacing 2^-24, ties at odd multiples of 2^-25
        k = torch.arange(-2048, 2048).double()
        x = torch.cat([x, k * 2.0 ** -25, k * 2.0 ** -24 * 0.3, torch.tensor([2.0 ** -25, 3 * 2.0 ** -26, 2.0 ** -26])])
    else:
        x = torch.cat([x, torch.tensor([1e-39, 3e-40, 2.0 ** -133, 3 * 2.0 ** -134])])
    x32 = x.float()                                               # float32 inputs: torch rounds them once
    x = x32.double()
    got = nm.round_half(x, dtype)
    exp = _from_f32(x32, dtype)
    assert torch.equal(got, exp), x[(got != exp)][:8]
    if dtype == torch.float16:
        assert nm.round_half(torch.tensor([65520.0], dtype=torch.float64), dtype).item() == float("inf")
        assert nm.round_half(torch.tensor([65519.999], dtype=torch.float64), dtype).item() == 65504.0
        assert nm.round_half(torch.tensor([2.0 ** -25], dtype=torch.float64), dtype).item() == 0.0         # tie to the even zero
        assert nm.round_half(torch.tensor([3 * 2.0 ** -25], dtype=torch.float64), dtype).item() == 2.0 ** -23
    # one rounding from float64, where torch's bf16 conversion rounds twice (float64 -> float32 -> bf16)
    if dtype == torch.bfloat16:
        x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)        # just above the tie: up; via float32 it becomes the tie -> even (down)
        assert nm.round_half(x, dtype).item() == 1.0 + 2.0 ** -7
    assert torch.equal(nm.ulp(torch.tensor([1.0, 1.5, 2.0]), dtype), torch.tensor([2.0 ** (1 - p)] * 2 + [2.0 ** (2 - p)]).double())
    assert nm.ulp(torch.tensor([0.0]), dtype).item() == 2.0 ** (emin - p + 1)


def _case(dtype, seed=1, shape=(256, 512)):
    g = torch.Generator().manual_seed(seed)
    ref = torch.randn(*shape, generator=g).double() * 3
    return ref, nm.round_half(ref, dtype).to(dtype)


def _loc(msg):
    m = re.search(r"worst element \[(\d+), (\d+)\]", msg)
    return int(m.group(1)), int(m.group(2))


@pytest.mark.parametrize("dtype", HALF)
def test_checker_passes_correctly_rounded_outputs(dtype):
    ref, got = _case(dtype)
    info = nm.check(got, ref, 0.5 * nm.ulp(ref, dtype), what="rounded")
    assert info["n_bad"] == 0 and 0.2 < info["worst_block_rms"] < nm.RMS_LIMIT
    nm.check_exact(got, nm.round_half(ref, dtype))


@pytest.mark.parametrize("dtype", HALF)
def test_checker_flags_one_element_two_ulps_off(dtype):
    ref, got = _case(dtype)
    bad = got.double().clone()
    bad[77, 301] += 2 * nm.ulp(bad[77, 301:302], dtype)[0]
    with pytest.raises(AssertionError) as e:
        nm.check(bad.to(dtype), ref, 0.5 * nm.ulp(ref, dtype), what="2 ulp")
    assert _loc(str(e.value)) == (77, 301) and "worst row 77" in str(e.value) and "worst column 301" in str(e.value)
    assert "rows 64..79 cols 288..303" in str(e.value)


@pytest.mark.parametrize("dtype", HALF)
def test_checker_flags_a_block_with_a_missing_k_tile(dtype):
    """one 16 x 16 output block computed without one of its K tiles: A @ W^T over K = 256, tile k = 64..127 dropped there"""
    g = torch.Generator().manual_seed(2)
    A = torch.randn(128, 256, generator=g).double()
    W = torch.randn(96, 256, generator=g).double() / 16
    ref = A @ W.T
    bad = ref.clone()
    bad[32:48, 48:64] -= A[32:48, 64:128] @ W[48:64, 64:128].T
    with pytest.raises(AssertionError) as e:
        nm.check(nm.round_half(bad, dtype).to(dtype), ref, 0.5 * nm.ulp(ref, dtype), what="K tile")
    s = str(e.value)
    r, c = _loc(s)
    assert 32 <= r < 48 and 48 <= c < 64 and "rows 32..47 cols 48..63" in s


@pytest.mark.parametrize("dtype", HALF)
def test_checker_flags_a_row_without_its_bias(dtype):
    ref, _ = _case(dtype)
    bias = torch.linspace(-2, 2, ref.shape[1]).double()
    full = ref + bias
    bad = full.clone()
    bad[200] -= bias
    with pytest.raises(AssertionError) as e:
        nm.check(nm.round_half(bad, dtype).to(dtype), full, 0.5 * nm.ulp(full, dtype), what="bias")
    assert "worst row 200" in str(e.value) and _loc(str(e.value))[0] == 200


@pytest.mark.parametrize("dtype", HALF)
def test_checker_flags_two_swapped_columns(dtype):
    ref, got = _case(dtype)
    bad = got.clone()
    bad[:, [5, 130]] = bad[:, [130, 5]]
    with pytest.raises(AssertionError) as e:
        nm.check(bad, ref, 0.5 * nm.ulp(ref, dtype), what="swap")
    assert _loc(str(e.value))[1] in (5, 130) and re.search(r"worst column (5|130)\b", str(e.value))


@pytest.mark.parametrize("dtype", HALF)
def test_checker_flags_truncation_instead_of_round_to_nearest_even(dtype):
    """truncation (round toward zero) is at most 1 ulp off: the elementwise half-ulp bound catches it, and even under a
    1-ulp bound (the GELU epilogue's) the RMS gate does -- truncation's RMS is ~0.58 ulp, rounding's 0.29"""
    ref, _ = _case(dtype)
    trunc = torch.trunc(ref / nm.ulp(ref, dtype)) * nm.ulp(ref, dtype)
    assert torch.equal(trunc.to(dtype).double(), trunc)
    with pytest.raises(AssertionError, match="elementwise"):
        nm.check(trunc.to(dtype), ref, 0.5 * nm.ulp(ref, dtype), what="trunc")
    with pytest.raises(AssertionError, match="RMS gate"):
        nm.check(trunc.to(dtype), ref, nm.ulp(ref, dtype), what="trunc, 1-ulp bound")
    # the same under the exact (tie) reference
    with pytest.raises(AssertionError):
        nm.check_exact(trunc.to(dtype), ref)


def test_checker_flags_fp16_overflow_stored_as_max():
    ref = torch.full((32, 32), 1000.0, dtype=torch.float64)
    ref[9, 17] = 65520.0                       # rounds to +inf in fp16
    ref[3, 4] = -65536.0
    got = nm.round_half(ref, torch.float16).to(torch.float16)
    nm.check_exact(got, ref)                   # inf where inf is due
    bad = got.clone()
    bad[9, 17] = 65504.0                       # saturated instead of overflowing
    with pytest.raises(AssertionError) as e:
        nm.check_exact(bad, ref, what="saturation")
    assert _loc(str(e.value)) == (9, 17)


def test_round_half_float32_equals_torch_float():
    """float32 in the same table: round_half(x64, float32) == x64.float() (torch's one RNE step from float64) on random
    values over the whole exponent range, exact ties, subnormals (spacing 2^-149, ties at odd multiples of 2^-150) and values
    past FLT_MAX (from FLT_MAX + ulp/2 = 2^128 - 2^103 on: inf)"""
    f32 = torch.float32
    g = torch.Generator().manual_seed(3)
    n = 8192
    sgn = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    # exact ties: (m + 1/2) ulp with a 24-bit significand m, and just above / below them (float64 has 29 more bits)
    e = torch.randint(-120, 120, (n,), generator=g).double()
    m = torch.randint(2 ** 23, 2 ** 24, (n,), generator=g).double()
    ties = (m + 0.5) * torch.exp2(e - 23) * sgn
    near = torch.cat([ties * (1 + 2.0 ** -40), ties * (1 - 2.0 ** -40)])
    rnd = torch.randn(n, generator=g).double() * torch.exp2(torch.randint(-140, 128, (n,), generator=g).double())
    k = torch.arange(-4096, 4096).double()
    sub = torch.cat([k * 2.0 ** -150, k * 2.0 ** -149 * 0.3, k * 2.0 ** -140 + 2.0 ** -150])     # ties, inexact, subnormal
    fmax = (2.0 - 2.0 ** -23) * 2.0 ** 127
    big = torch.tensor([fmax, fmax + 2.0 ** 102, fmax + 2.0 ** 103 - 2.0 ** 80, fmax + 2.0 ** 103, 2.0 ** 128, 1e300, 1e39])
    big = torch.cat([big, -big])
    x = torch.cat([ties, near, rnd, sub, big, torch.tensor([0.0, -0.0, 2.0 ** -151, 3 * 2.0 ** -151])])
    got = nm.round_half(x, f32)
    exp = x.float().double()
    assert torch.equal(got, exp), (x[got != exp][:8], got[got != exp][:8], exp[got != exp][:8])
    assert nm.round_half(torch.tensor([fmax + 2.0 ** 103], dtype=torch.float64), f32).item() == float("inf")
    assert nm.round_half(torch.tensor([fmax + 2.0 ** 103 - 2.0 ** 80], dtype=torch.float64), f32).item() == fmax
    assert nm.round_half(torch.tensor([2.0 ** -150], dtype=torch.float64), f32).item() == 0.0          # tie to the even zero
    assert nm.round_half(torch.tensor([3 * 2.0 ** -150], dtype=torch.float64), f32).item() == 2.0 ** -148
    assert nm.ulp(torch.tensor([1.0]), f32).item() == 2.0 ** -23 and nm.ulp(torch.tensor([0.0]), f32).item() == 2.0 ** -149
    # the checker on float32 outputs: exact where exact, one float32 ulp flagged and located
    ref = torch.randn(64, 96, generator=g).double()
    got32 = ref.float()
    nm.check_exact(got32, ref, what="f32")
    bad = got32.clone()
    bad[10, 20] = torch.nextafter(bad[10, 20], torch.tensor(float("inf")))
    with pytest.raises(AssertionError) as ei:
        nm.check_exact(bad, ref, what="f32 1 ulp")
    assert _loc(str(ei.value)) == (10, 20)
