"""numpy reference of the packed twins' block walk and byte layout (kernels_pack.hip.h), written from
the format description alone: which elements a block holds, which blocks need an escape plane in
the 26-bit format, and how many bytes a tile takes in either format."""
import numpy as np

QUAD = 256 * 12          # a k-quad: 256 lanes x three dwords
CODE = {28: 256 * 8, 26: 256 * 4}   # the code plane: two dwords / one dword per lane
ESC_PLANE = 256 * 4      # escape plane of one block (format 26)
SECOND_COPY_ORDER = {4: (2, 3, 0, 1), 3: (2, 0, 1)}   # modes of the transposed copy, fastest first


def tile_bytes(fmt, J):
    """bytes of one (row tile, batch): per k-block of 16 reduction indices the code plane, then one
    quad per 4 indices — of a short last block only the quads that reach below J"""
    total = 0
    for kb in range((J + 15) // 16):
        quads = min(4, (J - 16 * kb + 3) // 4)
        total += CODE[fmt] + quads * QUAD
    return total


def layout_elements(V, layout):
    """the fp32 elements of a resident layout in storage order"""
    V = np.asarray(V)
    if layout == "tensor":
        return np.float32(V).ravel(order="F")
    assert layout == "second (transposed) copy", layout
    return np.float32(V).transpose(SECOND_COPY_ORDER[V.ndim]).ravel(order="F")


def top_bytes(flat):
    return (np.ascontiguousarray(flat, dtype=np.float32).view(np.uint32) >> 24).astype(np.int64)


def block_index(L, J, T, mtile, kb, batch):
    """block order: k-blocks of a tile consecutive, row tiles fastest, then batches"""
    return (batch * ((L + 255) // 256) + mtile) * ((J + 15) // 16) + kb


def block_members(L, J, T, mtile, kb, batch):
    """storage indices (m + L*(k + J*batch)) of the elements of one block"""
    m = np.arange(256 * mtile, min(L, 256 * mtile + 256))
    k = np.arange(16 * kb, min(J, 16 * kb + 16))
    return (m[:, None] + L * (k[None, :] + J * batch)).ravel()


def block_spreads(flat, L, J, T):
    """max - min top byte of every block, in block order"""
    tb = top_bytes(flat).reshape(T, J, L)
    n_mtiles, nkb = (L + 255) // 256, (J + 15) // 16
    out = np.zeros((T, n_mtiles, nkb), dtype=np.int64)
    for mt in range(n_mtiles):
        for kb in range(nkb):
            blk = tb[:, 16 * kb:16 * kb + 16, 256 * mt:256 * mt + 256].reshape(T, -1)
            out[:, mt, kb] = blk.max(axis=1) - blk.min(axis=1)
    return out.ravel()


def escape_blocks(flat, L, J, T):
    """blocks whose codes need more than two bits (spread 4..15); None if a block is beyond the window"""
    s = block_spreads(flat, L, J, T)
    return None if (s >= 16).any() else int((s >= 4).sum())


def choose_format(mode, spread, escapes, blocks):
    """PPALS_PACK_LAYOUT rule: 1 -> 28, 2 -> 26, otherwise 26 while escapes <= blocks/16, else 28;
    0: refused (a block at or beyond the window of 16)"""
    if spread < 0 or spread >= 16:
        return 0
    if mode == 1:
        return 28
    fits = escapes < (1 << 24) - 1
    if mode == 2:
        return 26 if fits else 0
    return 26 if fits and 16 * escapes <= blocks else 28


def perm(hi, lo, sel):
    """v_perm_b32: result byte i by selector byte i: 0..3 byte of lo, 4..7 byte of hi, 0x0c zero"""
    both = (hi << 32) | lo
    r = 0
    for i in range(4):
        s = (sel >> (8 * i)) & 0xff
        assert s < 8 or s == 0x0c, hex(s)
        b = ((both >> (8 * s)) & 0xff) if s < 8 else 0
        r |= b << (8 * i)
    return r
