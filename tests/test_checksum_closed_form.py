"""tests/checksum_closed_form.py against a brute-force numpy reference that
takes the same ``wrap``, so that the closed form has been across a weight
wrap, on sizes numpy can hold, before the 16 GiB tests trust it across the
real one."""

import numpy as np
import pytest

from checksum_closed_form import MASK64, WRAP, expected, vector_sentinels, weight_sum, word_bytes

SMALL_WRAPS = [1024, 4096]
FILLS = [0x00, 0xFF]


def brute_force(nbytes, fill_byte, sparse, wrap):
    """(s0, s1) as the protocol defines them, with ``wrap`` for 2^32: build
    the bytes, pad to 4, view as little-endian u32, widen to u64, wrapping
    sums."""
    data = bytearray([fill_byte]) * nbytes
    for offset, value in sparse.items():
        data[offset] = value
    data += b"\0" * (-nbytes % 4)
    words = np.frombuffer(bytes(data), dtype="<u4").astype(np.uint64)
    weight = (np.arange(len(words), dtype=np.uint64) % np.uint64(wrap)) + np.uint64(1)
    with np.errstate(over="ignore"):
        return (
            int(words.sum(dtype=np.uint64)),
            int((words * weight).sum(dtype=np.uint64)),
        )


def straddling_sizes(wrap, multiples):
    """Byte counts around ``k * wrap`` words: one word less, exact, one word
    more, each with 1 to 3 bytes less and more."""
    sizes = set()
    for k in multiples:
        for dword in (-1, 0, 1):
            for dbyte in range(-3, 4):
                n = 4 * (k * wrap + dword) + dbyte
                if n >= 0:
                    sizes.add(n)
    return sorted(sizes)


def sparse_around_wraps(nbytes, wrap):
    """A few bytes on both sides of every wrap inside the buffer, and the
    last byte; values that are neither fill byte."""
    offsets = set()
    for k in range(1, 5):
        edge = 4 * k * wrap
        offsets.update((edge - 7, edge - 4, edge - 1, edge, edge + 2, edge + 5))
    offsets.add(nbytes - 1)
    offsets.add(0)
    return {o: 1 + (o * 37 + 11) % 254 for o in sorted(offsets) if 0 <= o < nbytes}


def test_hand_computed_case():
    """Words 1, 2, 3 and a padded last word 0x0504, as in test_arg_checksum."""
    sparse = {0: 1, 4: 2, 8: 3, 12: 4, 13: 5}
    want = (1 + 2 + 3 + 0x0504, 1 * 1 + 2 * 2 + 3 * 3 + 0x0504 * 4)
    assert expected(14, 0, sparse) == want
    assert brute_force(14, 0, sparse, WRAP) == want
    # with a wrap of 2 words the weights are 1, 2, 1, 2
    want = (1 + 2 + 3 + 0x0504, 1 * 1 + 2 * 2 + 3 * 1 + 0x0504 * 2)
    assert expected(14, 0, sparse, wrap=2) == want
    assert brute_force(14, 0, sparse, 2) == want


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("wrap", SMALL_WRAPS)
def test_closed_form_across_small_wraps(wrap, fill):
    for n in straddling_sizes(wrap, (0, 1, 2, 3)):
        want = brute_force(n, fill, {}, wrap)
        assert expected(n, fill, {}, wrap) == want, (wrap, fill, n, "no sparse bytes")
        sparse = sparse_around_wraps(n, wrap)
        want = brute_force(n, fill, sparse, wrap)
        assert expected(n, fill, sparse, wrap) == want, (wrap, fill, n, sorted(sparse))


@pytest.mark.parametrize("fill", FILLS)
def test_closed_form_at_the_protocol_wrap_on_small_sizes(fill):
    """wrap = 2^32 where numpy can follow: around 0 words, and at a few
    thousand bytes."""
    for n in straddling_sizes(WRAP, (0,)) + [4096, 4099, 65535]:
        sparse = sparse_around_wraps(n, 1024)
        assert expected(n, fill, sparse) == brute_force(n, fill, sparse, WRAP), (fill, n)


@pytest.mark.parametrize("fill", FILLS)
def test_closed_form_at_the_protocol_wrap_by_cycles(fill):
    """wrap = 2^32 around 1, 2 and 3 cycles, where no array can follow.  Every
    cycle restarts the weights at 1, so the pair of the whole buffer is the
    sum of the pairs of its cycles, each taken as a buffer of its own that
    never wraps (a path the tests above pin against numpy)."""
    never = 1 << 62
    cycle_bytes = 4 * WRAP
    for n in straddling_sizes(WRAP, (1, 2, 3)):
        sparse = sparse_around_wraps(n, WRAP)
        s0 = s1 = 0
        for start in range(0, n, cycle_bytes):
            size = min(cycle_bytes, n - start)
            part = {o - start: v for o, v in sparse.items() if start <= o < start + size}
            p0, p1 = expected(size, fill, part, wrap=never)
            s0 += p0
            s1 += p1
        assert expected(n, fill, sparse) == (s0 & MASK64, s1 & MASK64), (fill, n)


def test_weight_sum_is_the_plain_sum():
    for wrap in (1, 2, 7, 1024):
        for words in (0, 1, wrap - 1, wrap, wrap + 1, 3 * wrap + 5):
            assert weight_sum(words, wrap) == sum(i % wrap + 1 for i in range(words))


def test_sentinels_sit_where_the_docstrings_say():
    n = 4 * WRAP + 65536 + 7
    sparse = vector_sentinels(n)
    assert all(0 <= o < n for o in sparse)
    words = {o // 4 for o in sparse}
    assert set(range(WRAP - 4, WRAP + 4)) <= words  # both vectors, every position
    assert {0, 10, (n - 1) // 4, (n - 7) // 4} <= words
    assert all(sparse[o] == 0xFF for o in word_bytes(WRAP - 1, 0))
    # a weight that is 2^32 too large after the boundary must show modulo 2^64
    low = sum(v << (8 * (o % 4)) for o, v in sparse.items() if o // 4 >= WRAP)
    assert low % (1 << 32) != 0


def test_bad_arguments_are_refused():
    with pytest.raises(ValueError):
        expected(8, 0, {8: 1})
    with pytest.raises(ValueError):
        expected(8, 256)
