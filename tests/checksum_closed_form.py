"""The argument checksum in closed form, for buffers too large for numpy.

docs/PROTOCOL.md: view the ``n`` bytes as little-endian u32 words ``w_i``,
the last one zero-padded; ``s0 = sum w_i`` and ``s1 = sum w_i * ((i mod
2^32) + 1)``, both modulo 2^64.  :func:`expected` computes that pair in
Python integers for a buffer that is one fill byte everywhere except at a
few given offsets, so it costs the same at 16 GiB as at 16 bytes.  ``wrap``
is 2^32 in the protocol; it is a parameter so that test_checksum_closed_form
can run this code across several wraps on sizes numpy can hold before the
large tests trust it across the real one.

Also here, because the host and the device tests at the 2^32-word boundary
must describe the same content: the sentinel bytes of those tests and the
private anonymous mapping that holds them on the host.
"""

import mmap

MASK64 = (1 << 64) - 1
WRAP = 1 << 32  # words per weight cycle in the protocol


def weight_sum(words: int, wrap: int) -> int:
    """Sum of ``(i mod wrap) + 1`` for ``i`` in ``range(words)``: one
    arithmetic series per full cycle and one for the partial cycle."""
    cycles, rest = divmod(words, wrap)
    return cycles * (wrap * (wrap + 1) // 2) + rest * (rest + 1) // 2


def expected(nbytes: int, fill_byte: int, sparse=None, wrap: int = WRAP):
    """``(s0, s1)`` of ``nbytes`` of ``fill_byte`` with the bytes in
    ``sparse`` (``{byte offset: byte value}``) written over them."""
    if nbytes < 0 or not 0 <= fill_byte <= 0xFF or wrap < 1:
        raise ValueError("bad arguments")
    full, tail = divmod(nbytes, 4)
    word = fill_byte * 0x01010101
    tail_word = fill_byte * (0x01010101 & ((1 << (8 * tail)) - 1))  # zero-extended
    s0 = word * full + tail_word
    s1 = word * weight_sum(full, wrap) + tail_word * (full % wrap + 1)
    for offset, value in (sparse or {}).items():
        if not 0 <= offset < nbytes or not 0 <= value <= 0xFF:
            raise ValueError(f"sparse byte {value!r} at {offset!r} outside the buffer")
        delta = (value - fill_byte) << (8 * (offset % 4))
        s0 += delta
        s1 += delta * ((offset // 4) % wrap + 1)
    return s0 & MASK64, s1 & MASK64


def word_bytes(index: int, value: int) -> dict:
    """The four bytes of little-endian u32 ``value`` at word ``index``."""
    return {4 * index + k: (value >> (8 * k)) & 0xFF for k in range(4)}


# The smallest size at which an implementation that forgets the wrap can
# differ: 16 GiB, one more 64 KiB so that whole device vectors, and many of
# them, lie past the boundary, and a ragged end.
BOUNDARY_BYTES = 4 * WRAP + 65536


def boundary_sentinels(nbytes: int) -> dict:
    """Sparse bytes for a buffer of zeros that crosses the 2^32-word
    boundary once: the first word, an early one, the last word of the first
    cycle (weight 2^32, all ones, so its product is the largest there is),
    the first two of the second cycle (weights 1 and 2), and the last byte.
    The words after the boundary have non-zero low halves and so does their
    sum: a weight that is too large by 2^32 cannot vanish modulo 2^64."""
    if nbytes <= 4 * (WRAP + 2):
        raise ValueError("the buffer does not cross the boundary")
    sparse = {}
    sparse.update(word_bytes(0, 0x01020304))
    sparse.update(word_bytes(10, 0xDEADBEEF))
    sparse.update(word_bytes(WRAP - 1, 0xFFFFFFFF))
    sparse.update(word_bytes(WRAP, 0x9E3779B9))
    sparse.update(word_bytes(WRAP + 1, 0x12345678))
    sparse[nbytes - 1] = 0xC3
    return sparse


def vector_sentinels(nbytes: int) -> dict:
    """:func:`boundary_sentinels` plus, for kernels that read 16-byte
    vectors: a distinct word in each of the four positions of the vector
    that ends the first cycle and of the vector that begins the second, and
    a byte in the first word of the ragged end (the last byte sits in its
    last word when the end is 5 to 7 bytes long)."""
    sparse = {}
    for k in range(8):
        sparse.update(word_bytes(WRAP - 4 + k, 0x0F1E2D3C + 0x11111111 * k))
    sparse.update(boundary_sentinels(nbytes))
    sparse[nbytes - nbytes % 16] = 0x5A
    return sparse


def sparse_mapping(nbytes: int, sparse: dict):
    """``nbytes`` of zeros with ``sparse`` written over them, as a private
    anonymous mapping without reserved swap: only the written pages take
    memory, every other read sees the kernel's zero page.  (A shared
    anonymous mapping would allocate each page it reads.)"""
    flags = mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS | getattr(mmap, "MAP_NORESERVE", 0)
    buf = mmap.mmap(-1, nbytes, flags=flags)
    for offset, value in sparse.items():
        buf[offset] = value
    return buf
