"""The host half of the argument checksum at the 2^32-word boundary, where
the weight of ``s1`` wraps: ``native_io.checksum`` (csp_io.h) and
``workers.threaded_checksum`` over 16 GiB + 64 KiB + 3 bytes against the
closed form of tests/checksum_closed_form.py.

The buffer is a private anonymous mapping of zeros with a few sentinel
bytes, so it takes a few pages of memory; each pass still reads all of it
(seconds, not milliseconds), hence three passes and no more."""

import gc
import resource

import pytest

from checksum_closed_form import BOUNDARY_BYTES, WRAP, boundary_sentinels, expected, sparse_mapping

from covalent_ssh_plugin_amd.remote import workers
from covalent_ssh_plugin_amd.transport import native_io

N = BOUNDARY_BYTES + 3
RSS_GROWTH_LIMIT_KIB = 1 << 20  # 1 GiB; ru_maxrss is in KiB on Linux


def _maxrss_kib():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss


@pytest.fixture(scope="module")
def boundary():
    """(mapping, sentinels, closed form, ru_maxrss before the mapping)."""
    assert native_io.load() is not None, "libcsp_io.so was not built"
    before = _maxrss_kib()
    sparse = boundary_sentinels(N)
    buf = sparse_mapping(N, sparse)
    yield buf, sparse, expected(N, 0x00, sparse), before
    gc.collect()  # ctypes carriers of the passes still export the mapping
    try:
        buf.close()
    except BufferError:
        pass  # unmapped with the last export instead


def test_sentinels_are_in_the_mapping(boundary):
    buf, sparse, want, _before = boundary
    assert len(buf) == N == 4 * WRAP + 65536 + 3
    assert bytes(buf[0:4]) == bytes([0x04, 0x03, 0x02, 0x01])
    assert bytes(buf[4 * WRAP - 4 : 4 * WRAP]) == b"\xff" * 4
    assert buf[N - 1] == sparse[N - 1] != 0
    # by hand: the all-ones word has weight 2^32, the next word weight 1
    by_hand = (
        0x01020304 * 1 + 0xDEADBEEF * 11 + 0xFFFFFFFF * (1 << 32)
        + 0x9E3779B9 * 1 + 0x12345678 * 2 + (0xC3 << 16) * (16384 + 1)
    )
    assert (N - 1) // 4 - WRAP == 16384 and (N - 1) % 4 == 2
    assert want[1] == by_hand % (1 << 64)


def test_native_checksum_wraps_at_2_to_32_words(boundary):
    buf, _sparse, want, before = boundary
    assert native_io.checksum(buf) == want
    assert _maxrss_kib() - before < RSS_GROWTH_LIMIT_KIB, "the pass touched its pages"


@pytest.mark.parametrize("chunk", [workers.ARG_CACHE_CHUNK, 16 << 30],
                         ids=["default-chunk", "chunk-16GiB"])
def test_threaded_checksum_wraps_at_2_to_32_words(boundary, chunk):
    """At 16 GiB a piece begins exactly at the boundary: its word offset
    modulo 2^32 is 0, not 2^32."""
    buf, _sparse, want, before = boundary
    assert (4 * WRAP) % chunk == 0
    assert workers.threaded_checksum(buf, chunk) == want
    assert _maxrss_kib() - before < RSS_GROWTH_LIMIT_KIB, "the pass touched its pages"
