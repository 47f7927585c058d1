"""The stand-alone Bitmap operations in plain numpy integers: the yardstick of pack_kernel, diff_weights_kernel and
delta_pages_kernel (csrc/iiv_bitmap.hip) and of screen.Bitmap's packed / apply / diff_weights / compute_delta_page.  No device.

Written from include/iivision.h, DESIGN sections 1 and 3 and the bit layouts transcoder/screen.py documents.

A packed column is header | body | footer, least significant bit first:

    HGR   22 bits   hhh aaaaaaaA Bbbbbbbb fff     a = the even byte's bits 0..7 at bits 3..10 (A, its palette bit, at 10);
                                                  the odd byte's palette bit B at 11 and its data bits 0..6 at 12..18
    DHGR  34 bits   hhh + 4 x 7 + fff             aux even, main even, aux odd, main odd at bits 3, 10, 17, 24; bit 7 of a
                                                  screen byte is not displayed and does not enter

    header (bits 0..2) comes from the column to the LEFT:   HGR its odd byte's data bits 5, 6 (column bits 17, 18) at 0, 1 and
                                                            palette bit (11) at 2; DHGR its column bits 28..30
    footer (top 3 bits) comes from the column to the RIGHT: HGR its even byte's palette bit (10) at 19 and data bits 0, 1
                                                            (3, 4) at 20, 21; DHGR its column bits 3..5 at 31..33
    column 0 of a page has a zero header and column 127 a zero footer: a page never sees its neighbour pages.

Byte offset o of the screen byte at page offset y:  HGR y & 1;  DHGR 2 (y & 1) + (0 for the aux bank, 1 for main).
The window of byte o (what the edit-distance table is indexed by):  (column & BYTE_MASKS[o]) >> BYTE_SHIFTS[o], MASKED_BITS wide.
The table is a host uint16 array (num_offsets, 2 ** (2 * MASKED_BITS)), entry [o][(source window << MASKED_BITS) + target window].

compute_delta_page is taken literally: `content` goes into byte o of EVERY column of the page, then headers or footers of
the whole row are rebuilt from the neighbour column with wrap-around (column 127's right neighbour is column 0), then the
windows are cut.  delta_pages_kernel skips the rebuild, arguing that it only changes bits outside byte o's window; this model
must not, that claim is what the tests hold it to.
"""
import numpy as np

HGR, DHGR = 0, 1
U = np.uint64

HEADER_BITS = {HGR: 3, DHGR: 3}
BODY_BITS = {HGR: 16, DHGR: 28}
FOOTER_BITS = {HGR: 3, DHGR: 3}
MASKED_BITS = {HGR: 14, DHGR: 13}
NUM_OFFSETS = {HGR: 2, DHGR: 4}
BYTE_SHIFTS = {HGR: (0, 8), DHGR: (0, 7, 14, 21)}
BYTE_MASKS = {m: tuple(((1 << MASKED_BITS[m]) - 1) << s for s in BYTE_SHIFTS[m]) for m in (HGR, DHGR)}
# (first bit, width) of the field masked_update replaces, per byte offset
BYTE_FIELD = {HGR: ((3, 8), (11, 8)), DHGR: ((3, 7), (10, 7), (17, 7), (24, 7))}


def _u(a):
    return np.asarray(a).astype(U)


def body(mode, main, aux=None):
    """(..., 32, 256) screen bytes -> (..., 32, 128) uint64 column bodies (header and footer bits zero)"""
    main = _u(main)
    even, odd = main[..., 0::2], main[..., 1::2]
    if mode == HGR:
        return (even << U(3)) | ((odd >> U(7)) << U(11)) | ((odd & U(0x7f)) << U(12))
    aux = _u(aux)
    a_even, a_odd = aux[..., 0::2] & U(0x7f), aux[..., 1::2] & U(0x7f)
    return (a_even << U(3)) | ((even & U(0x7f)) << U(10)) | (a_odd << U(17)) | ((odd & U(0x7f)) << U(24))


def make_header(mode, col):
    """the header a column hands to its RIGHT neighbour"""
    col = _u(col)
    if mode == HGR:
        return (((col >> U(11)) & U(1)) << U(2)) | ((col >> U(17)) & U(3))
    return (col >> U(28)) & U(7)


def make_footer(mode, col):
    """the footer a column hands to its LEFT neighbour"""
    col = _u(col)
    if mode == HGR:
        return (((col >> U(10)) & U(1)) | (((col >> U(3)) & U(3)) << U(1))) << U(19)
    return ((col >> U(3)) & U(7)) << U(31)


def pack(mode, main, aux=None):
    """(..., 32, 256) uint8 main (and aux for DHGR) -> (..., 32, 128) uint64; any leading dimensions"""
    b = body(mode, main, aux)
    out = b.copy()
    out[..., 1:] |= make_header(mode, b[..., :-1])
    out[..., :-1] |= make_footer(mode, b[..., 1:])
    return out


def byte_offset(mode, y, is_aux):
    if mode == HGR:
        assert not is_aux
        return y & 1
    return 2 * (y & 1) + (0 if is_aux else 1)


def byte_offsets(mode, is_aux):
    """the byte offsets of the even and of the odd page offsets of a bank"""
    return byte_offset(mode, 0, is_aux), byte_offset(mode, 1, is_aux)


def window(mode, packed, o):
    return (_u(packed) & U(BYTE_MASKS[mode][o])) >> U(BYTE_SHIFTS[mode][o])


def masked_update(mode, o, packed, content):
    """`content` (one byte, or an array that broadcasts against the columns) stored as byte o of every column; neighbours'
    headers and footers untouched"""
    content = np.asarray(content)
    assert ((content >= 0) & (content <= 255)).all()
    content = content.astype(U)
    at, width = BYTE_FIELD[mode][o]
    if mode == DHGR:
        field = content & U(0x7f)
    elif o == 0:
        field = content
    else:
        field = ((content & U(0x7f)) << U(1)) | (content >> U(7))        # the odd byte's palette bit sits below its data bits
    keep = ((1 << 64) - 1) ^ (((1 << width) - 1) << at)
    return (_u(packed) & U(keep)) | (field << U(at))


def fix_neighbours(mode, row, o):
    """the whole-array fix-up after a store to byte o of every column: byte 0 feeds the left neighbour's footer, the last byte
    the right neighbour's header; other bytes feed nothing.  Wraps around the row's ends."""
    row = _u(row)
    hb = HEADER_BITS[mode] + BODY_BITS[mode]
    if o == 0:
        return (row & U((1 << hb) - 1)) | make_footer(mode, np.roll(row, -1, axis=-1))
    if o == NUM_OFFSETS[mode] - 1:
        total = hb + FOOTER_BITS[mode]
        return (row & U(((1 << total) - 1) ^ 7)) | make_header(mode, np.roll(row, 1, axis=-1))
    return row


def diff_weights(mode, table, src_packed, tgt_packed, is_aux):
    """(..., 32, 128) packed source and target -> (..., 32, 256) int32: the table's distance of every byte's windows"""
    src, tgt = _u(src_packed), _u(tgt_packed)
    assert src.shape == tgt.shape
    out = np.empty(src.shape[:-1] + (256,), dtype=np.int32)
    bits = U(MASKED_BITS[mode])
    for k, o in enumerate(byte_offsets(mode, is_aux)):
        pair = (window(mode, src, o) << bits) + window(mode, tgt, o)
        out[..., k::2] = table[o][pair.astype(np.int64)]
    return out


def compute_delta_pages(mode, table, tgt_packed, pages, contents, dw_rows, is_aux):
    """the batched form the entry point takes: n (page, content) queries against one (32, 128) packed bitmap, (n, 256) rows to
    subtract -> (n, 256) int32.  Every query is worked out on its own whole row, literally: store, rebuild, cut, look up."""
    pages = np.asarray(pages, dtype=np.int64).reshape(-1)
    assert ((pages >= 0) & (pages <= 31)).all()
    contents = np.asarray(contents).reshape(-1, 1)
    rows = _u(tgt_packed)[pages]                                          # (n, 128): each query's own copy of its page
    out = np.empty((len(pages), 256), dtype=np.int32)
    bits = U(MASKED_BITS[mode])
    for k, o in enumerate(byte_offsets(mode, is_aux)):
        stored = fix_neighbours(mode, masked_update(mode, o, rows, contents), o)
        pair = (window(mode, stored, o) << bits) + window(mode, rows, o)
        out[:, k::2] = table[o][pair.astype(np.int64)]
    return out - np.asarray(dw_rows, dtype=np.int32).reshape(len(pages), 256)


def compute_delta_page(mode, table, tgt_packed, page, content, dw_row, is_aux):
    """(32, 128) packed bitmap, one page, one content byte, that page's (256,) row -> (256,) int32"""
    return compute_delta_pages(mode, table, tgt_packed, [page], [content], np.asarray(dw_row).reshape(1, 256), is_aux)[0]


def apply(mode, packed, main, aux, page, offset, is_aux, value):
    """one store, in place, as Bitmap.apply does it: the column's byte, the one neighbour it feeds (not across the page's
    ends), the memory map"""
    o = byte_offset(mode, offset, is_aux)
    col = offset // 2
    row = packed[page]
    row[col] = masked_update(mode, o, row[col], value)
    hb = HEADER_BITS[mode] + BODY_BITS[mode]
    if o == 0 and col > 0:
        row[col - 1] = (row[col - 1] & U((1 << hb) - 1)) | make_footer(mode, row[col])
    elif o == NUM_OFFSETS[mode] - 1 and col < 127:
        total = hb + FOOTER_BITS[mode]
        row[col + 1] = (row[col + 1] & U(((1 << total) - 1) ^ 7)) | make_header(mode, row[col])
    (aux if is_aux else main)[page, offset] = value


# ---- inputs the tests share ----------------------------------------------------------------------------------------------

def random_screens(seed, n):
    """(main, aux), each (n, 32, 256) uint8 with all 8 bits in use, every screen different, and a non-zero byte at offsets 0, 1,
    254 and 255 of every page (the bytes the page-edge columns are made of)"""
    rng = np.random.default_rng([int(seed), 11])
    out = rng.integers(0, 256, (2, n, 32, 256), dtype=np.uint8)
    edge = out[..., [0, 1, 254, 255]]
    out[..., [0, 1, 254, 255]] = np.where(edge == 0, np.uint8(0x81), edge)
    return out[0], out[1]


def edge_feeding_screens(mode):
    """(main, aux) of one screen whose neighbouring columns differ in exactly the bits that feed headers and footers: the
    bytes alternate, column by column, between a value and the value with those bits flipped"""
    col = np.arange(128)
    page = np.arange(32)[:, None]
    main = np.zeros((32, 256), np.uint8)
    aux = np.zeros((32, 256), np.uint8)
    flip = (col + page) & 1
    if mode == HGR:
        # even byte: data bits 0, 1 and the palette bit feed the left footer; odd byte: data bits 5, 6 and the palette bit
        main[:, 0::2] = ((0x2c + 7 * page) & 0x7c) ^ (flip * 0x83)
        main[:, 1::2] = ((0x15 + 3 * page) & 0x1f) ^ (flip * 0xe0)
    else:
        # aux even byte: bits 0..2 feed the left footer; main odd byte: bits 4..6 feed the right header
        aux[:, 0::2] = ((0x28 + 5 * page) & 0x78) | (flip * 0x07) | (0x80 * (page & 1))
        main[:, 1::2] = ((0x05 + page) & 0x0f) | (flip * 0x70) | (0x80 * (page & 1))
        main[:, 0::2] = 0x33 + page
        aux[:, 1::2] = 0x4c + page
    return main, aux
