"""Host tests (-m "not gpu") of the device 8-point RANSAC's sampler: the derivation of a sample from the generator outputs
at a fixed offset (vo_rng_choice8_from_raw -- the function the hypothesis kernel runs) against NumPy's own
Generator.choice, and the binding's new symbols."""
import ctypes as C

import numpy as np
import pytest

M32 = 0xFFFFFFFF


def raw_words(seed, n_words):
    """The generator's 32-bit stream: every 64-bit output split low half, high half."""
    r = np.random.PCG64(seed).random_raw((n_words + 1) // 2)
    w = np.empty(2 * r.size, np.uint32)
    w[0::2] = (r & np.uint64(M32)).astype(np.uint32)
    w[1::2] = (r >> np.uint64(32)).astype(np.uint32)
    return w


def numpy_choice_model(words, pos, n):
    """Generator.choice(n, 8, replace=False) read off the 32-bit stream from `pos` on, rejections included (Lemire's
    bounded draw; Floyd with the upper ends n-8 .. n-1; the shuffle with 7 .. 1): (sample, position behind it)."""
    def bounded(rng):
        nonlocal pos
        if rng == 0:
            return 0
        rex = rng + 1
        m = int(words[pos]) * rex
        pos += 1
        if (m & M32) < rex:
            thr = (M32 - rng) % rex
            while (m & M32) < thr:
                m = int(words[pos]) * rex
                pos += 1
        return m >> 32
    v = []
    for j in range(n - 8, n):
        val = bounded(j)
        v.append(j if val in v else val)
    for i in range(7, 0, -1):
        j = bounded(i)
        v[i], v[j] = v[j], v[i]
    return v, pos


@pytest.mark.parametrize("seed", [2023, 1, 7])
@pytest.mark.parametrize("n", [9, 37, 500, 1915, 2000, 4000])
def test_fixed_offset_derivation_equals_numpy_choice(seed, n):
    """2048 samples per (seed, n): the sample derived from outputs 15 i .. 15 i + 14 equals Generator.choice on every sample
    up to the stream's first truly rejected draw, and that sample is marked possibly rejected."""
    from vo import _native
    S = 2048
    words = raw_words(seed, 15 * S + 64)
    gen = np.random.Generator(np.random.PCG64(seed))
    pos, compared, first_reject = 0, 0, None
    for i in range(S):
        ref = gen.choice(n, 8, replace=False)
        model, nxt = numpy_choice_model(words, pos, n)
        assert list(ref) == model, "the test's model of NumPy's stream is wrong at sample %d" % i
        got, flag = _native.rng_choice8_from_raw(words[15 * i:15 * i + 15], n)
        if nxt - pos != 15:                       # NumPy's position departs from 15 per sample here
            assert flag == 1, "a truly rejected draw at sample %d is not marked" % i
            first_reject = i
            break
        assert list(got) == model, "sample %d" % i
        compared += 1
        pos = nxt
    print("seed %d n %d: %d samples equal, first truly rejected draw at %s" % (seed, n, compared, first_reject))
    assert compared == S or first_reject is not None
    assert compared >= 1


def marked_draws(words, n, S):
    """The marking rule on whole arrays: (S, 15) bool, entry [i, k] = draw k of sample i could have been rejected."""
    ranges = np.array([n - 8 + k for k in range(8)] + [7 - k for k in range(7)], np.uint64)
    raw = words[:15 * S].reshape(S, 15).astype(np.uint64)
    rex = ranges + np.uint64(1)
    return ((raw * rex) & np.uint64(M32)) < rex


def test_marked_and_rejected_draws_of_the_default_generator():
    """np.random.default_rng(2023), the first 2048 samples, every population size 9 .. 4000: which hold a possibly rejected
    draw; N = 3922 a truly rejected one at sample 18, N = 2215 at sample 801, N = 2911 one that is marked but not rejected
    at sample 412; no shuffle draw is ever marked."""
    from vo import _native
    S = 2048
    words = raw_words(2023, 15 * S + 64)
    ref = np.random.default_rng(2023).bit_generator.random_raw(4)
    assert np.array_equal(raw_words(2023, 8), np.stack([ref & np.uint64(M32), ref >> np.uint64(32)], 1).reshape(-1).astype(np.uint32))
    marked = {}
    for n in range(9, 4001):
        m = marked_draws(words, n, S)
        assert not m[:, 8:].any(), "a shuffle draw is marked at n = %d" % n
        if m.any():
            marked[n] = np.flatnonzero(m.any(axis=1))
    print("population sizes with a marked draw:", {n: v.tolist() for n, v in marked.items()})
    assert len(marked) == 13
    # the C function marks the same samples (all 2048 of every marked size, and of a few unmarked ones)
    for n in list(marked) + [9, 500, 2000, 4000]:
        flags = np.array([_native.rng_choice8_from_raw(words[15 * i:15 * i + 15], n)[1] for i in range(S)])
        assert np.array_equal(np.flatnonzero(flags), marked.get(n, np.zeros(0, np.int64))), n

    def first_departure(n):
        pos = 0
        for i in range(S):
            _, nxt = numpy_choice_model(words, pos, n)
            if nxt - pos != 15:
                return i
            pos = nxt
        return None
    assert marked[3922][0] == 18 and first_departure(3922) == 18
    assert marked[2215][0] == 801 and first_departure(2215) == 801
    assert marked[2911].tolist() == [412] and first_departure(2911) is None


def test_population_of_eight_is_refused():
    """At n = 8 the first Floyd draw has range 0 and NumPy consumes no output for it (14 per sample): not covered, and
    said so."""
    from vo import _native
    with pytest.raises(_native.VoError):
        _native.rng_choice8_from_raw(np.zeros(15, np.uint32), 8)
    gen = np.random.Generator(np.random.PCG64(5))
    words = raw_words(5, 64)
    ref = gen.choice(8, 8, replace=False)
    model, nxt = numpy_choice_model(words, 0, 8)
    assert list(ref) == model and nxt == 14


def test_new_symbols_and_structure_sizes():
    from vo import _native
    lib = C.CDLL(_native.lib_path())
    for name in ("vo_fundamental_ransac", "vo_rng_choice8_from_raw", "vo_rng_raw32_device", "vo_pipeline_bootstrap_lanes"):
        assert hasattr(lib, name), name
        assert name in _native._SIGS, name
    assert hasattr(_native.Context, "fundamental_ransac") and hasattr(_native.Pipeline, "bootstrap_lanes")
    assert C.sizeof(_native.BootstrapParams) == 72
    assert C.sizeof(_native.BootstrapResult) == 144
