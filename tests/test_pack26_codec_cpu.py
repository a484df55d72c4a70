"""The per-lane codec of the packed twins (csrc/pack_codec.h — the one definition the pack kernels,
the packed scans and this test share) on the host, through tests/pack26_shim: encode then decode
gives back the input words at every lane position, the host stand-in of the byte permute follows
the documented selector semantics, the tile sizes are those of the byte layout written out in
tests/pack26_ref.py, and the format choice is the stated rule."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pack26_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "pack26_shim", "build", "libpack26_shim.so")


@pytest.fixture(scope="module")
def shim():
    # (built on demand like the other shims: a tree whose tests/ lost its build products still runs this)
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "pack26_shim")])
    assert os.path.exists(LIB), "tests/pack26_shim did not build"
    lib = ctypes.CDLL(LIB)
    u32p, u8p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)
    lib.p26_pack_block.argtypes = [ctypes.c_int, u32p, ctypes.c_uint32, u8p, u8p]
    lib.p26_unpack_block.argtypes = [ctypes.c_int, u8p, u8p, ctypes.c_uint32, u32p]
    lib.p26_perm.argtypes = [ctypes.c_uint32] * 3
    lib.p26_perm.restype = ctypes.c_uint32
    lib.p26_tile_bytes.argtypes = [ctypes.c_int, ctypes.c_int64]
    lib.p26_tile_bytes.restype = ctypes.c_int64
    lib.p26_block_bytes.argtypes = [ctypes.c_int]
    lib.p26_choose_format.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64]
    lib.p26_side_word.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32]
    lib.p26_side_word.restype = ctypes.c_uint32
    return lib


def roundtrip(lib, fmt, base, codes, low):
    """codes, low: [256 threads, 4 quads, 4 rows]; returns the decoded words, the block, the plane"""
    u32p, u8p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)
    words = np.ascontiguousarray(((base + codes.astype(np.uint32)) << 24) | low, dtype=np.uint32)
    block = np.zeros(lib.p26_block_bytes(fmt), dtype=np.uint8)
    plane = np.zeros(ref.ESC_PLANE, dtype=np.uint8)
    out = np.zeros_like(words)
    lib.p26_pack_block(fmt, words.ctypes.data_as(u32p), base, block.ctypes.data_as(u8p), plane.ctypes.data_as(u8p))
    lib.p26_unpack_block(fmt, block.ctypes.data_as(u8p), plane.ctypes.data_as(u8p), base, out.ctypes.data_as(u32p))
    return words, out, block, plane


@pytest.mark.parametrize("base", [0, 1, 127, 240])
@pytest.mark.parametrize("fmt", [26, 28])
def test_encode_then_decode_gives_back_the_words(shim, fmt, base):
    rng = np.random.default_rng(fmt * 1000 + base)
    shape = (256, 4, 4)   # every lane position of the block, every quad, every row of the lane
    pos = np.arange(256 * 16, dtype=np.uint32).reshape(shape)
    for code in range(16):
        for codes in (np.full(shape, code, dtype=np.uint32), (pos + code) & 15):
            low = rng.integers(0, 1 << 24, shape, dtype=np.uint32)
            words, out, block, plane = roundtrip(shim, fmt, base, codes, low)
            assert np.array_equal(words, out), (fmt, base, code)
            if fmt == 26 and codes.max() < 4:   # codes 0..3 need no escape plane
                assert not plane.any(), (base, code)
    assert shim.p26_block_bytes(26) == 13312 and shim.p26_block_bytes(28) == 14336


def test_code_plane_bytes_of_format_26(shim):
    """byte jj of thread tid's code dword (at wave*256 + lane*4) holds the low code bits of row jj,
    quad u at bits 2u..2u+1; the escape plane holds the upper bits in the same arrangement"""
    rng = np.random.default_rng(3)
    codes = rng.integers(0, 16, (256, 4, 4), dtype=np.uint32)
    _, _, block, plane = roundtrip(shim, 26, 17, codes, np.zeros((256, 4, 4), dtype=np.uint32))
    for tid in (0, 1, 63, 64, 200, 255):
        for jj in range(4):
            off = (tid >> 6) * 256 + (tid & 63) * 4 + jj
            want_lo = sum(int(codes[tid, u, jj] & 3) << (2 * u) for u in range(4))
            want_hi = sum(int(codes[tid, u, jj] >> 2) << (2 * u) for u in range(4))
            assert (block[off], plane[off]) == (want_lo, want_hi), (tid, jj)


def test_side_words(shim):
    assert shim.p26_side_word(28, 0x7e, 0, 0) == 0x7e7e7e7e
    assert shim.p26_side_word(26, 0x7e, 0, 5) == 0x7e            # upper 24 bits zero: no escape plane
    assert shim.p26_side_word(26, 0x7e, 1, 0) == 0x7e | 1 << 8   # ordinal + 1
    assert shim.p26_side_word(26, 240, 1, 70000) == 240 | 70001 << 8


def test_host_permute_follows_the_selector_semantics(shim):
    rng = np.random.default_rng(11)
    sels = [0x04020100, 0x05020100, 0x06020100, 0x0c0c0703, 0x07030c0c, 0x03020100, 0x07060504, 0x0c0c0c0c,
            0x00010203, 0x04050607]
    for _ in range(50):
        hi, lo = (int(x) for x in rng.integers(0, 1 << 32, 2, dtype=np.uint64))
        for sel in sels:
            assert shim.p26_perm(hi, lo, sel) == ref.perm(hi, lo, sel), (hex(hi), hex(lo), hex(sel))


@pytest.mark.parametrize("J", [1, 4, 9, 16, 17, 40, 200])
def test_tile_bytes_of_both_formats(shim, J):
    for fmt in (28, 26):
        assert shim.p26_tile_bytes(fmt, J) == ref.tile_bytes(fmt, J), (fmt, J)
    if J == 200:   # the headline's tile
        assert shim.p26_tile_bytes(28, J) == 180224 and shim.p26_tile_bytes(26, J) == 166912


def test_format_choice_rule(shim):
    blocks = 406250
    cases = [(m, s, e) for m in (-1, 0, 1, 2, 7) for s in (-1, 0, 3, 4, 15, 16, 40)
             for e in (0, 19, blocks // 16, blocks // 16 + 1, blocks, (1 << 24) - 1)]
    for mode, spread, esc in cases:
        assert shim.p26_choose_format(mode, spread, esc, blocks) == ref.choose_format(mode, spread, esc, blocks), \
            (mode, spread, esc)
    # the stated rule, spelled out: refused at a spread of 16; forced formats; 1/16 is still 26 bits
    assert shim.p26_choose_format(-1, 16, 0, blocks) == 0 and shim.p26_choose_format(2, 16, 0, blocks) == 0
    assert shim.p26_choose_format(1, 3, 0, blocks) == 28 and shim.p26_choose_format(2, 15, blocks, blocks) == 26
    assert shim.p26_choose_format(-1, 4, 19, blocks) == 26                # the headline twin
    assert shim.p26_choose_format(-1, 15, 1600, 16 * 1600) == 26
    assert shim.p26_choose_format(-1, 15, 1601, 16 * 1600) == 28


def test_reference_counts_escape_blocks():
    """the numpy block walk itself, on a case small enough to check by hand: L = 260 rows (a partly
    filled second row tile), J = 20 (a short second k-block), T = 2 batches"""
    L, J, T = 260, 20, 2
    flat = np.ones(L * J * T, dtype=np.float32)
    assert ref.escape_blocks(flat, L, J, T) == 0
    hit = [(0, 0, 0), (1, 1, 0), (1, 0, 1)]          # (row tile, k-block, batch)
    for mt, kb, b in hit:
        flat[ref.block_members(L, J, T, mt, kb, b)[0]] = 2.0 ** -10    # 5 top bytes below 1.0
    s = ref.block_spreads(flat, L, J, T)
    assert s.shape == (2 * 2 * 2,) and ref.escape_blocks(flat, L, J, T) == 3
    assert sorted(np.nonzero(s)[0]) == sorted(ref.block_index(L, J, T, *h) for h in hit)
    flat[0] = 2.0 ** -40
    assert ref.escape_blocks(flat, L, J, T) is None
