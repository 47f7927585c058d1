"""tests/bitmap_model.py held on the CPU: against the reference-recorded g4 vectors and against the oracle, on inputs whose
conditions (all 8 bits in both modes, non-zero page-edge bytes) are asserted here, not assumed."""
import ctypes as C

import numpy as np
import pytest

import bitmap_model as M

MODES = [(M.HGR, "HGR"), (M.DHGR, "DHGR")]


def _banks(mode):
    return (0, 1) if mode == M.DHGR else (0,)


@pytest.fixture(scope="module")
def screens():
    return M.random_screens(41, 4)


def test_constants_are_the_documented_layouts(O):
    import screen
    for mode, cls in ((M.HGR, screen.HGRBitmap), (M.DHGR, screen.DHGRBitmap)):
        assert M.MASKED_BITS[mode] == int(cls.MASKED_BITS) == O.masked_bits(mode)
        assert M.NUM_OFFSETS[mode] == len(cls.BYTE_MASKS) == O.num_offsets(mode)
        assert list(M.BYTE_MASKS[mode]) == [int(v) for v in cls.BYTE_MASKS]
        assert list(M.BYTE_SHIFTS[mode]) == [int(v) for v in cls.BYTE_SHIFTS]
        assert (M.HEADER_BITS[mode], M.BODY_BITS[mode], M.FOOTER_BITS[mode]) == (int(cls.HEADER_BITS), int(cls.BODY_BITS), int(cls.FOOTER_BITS))
        for y in range(256):
            for ia in _banks(mode):
                assert M.byte_offset(mode, y, ia) == cls.byte_offset(y, bool(ia))


def test_input_conditions(screens, golden):
    main, aux = screens
    assert main.shape == aux.shape == (4, 32, 256) and main.dtype == np.uint8
    for bank in (main, aux):
        assert (bank >= 128).mean() >= 0.25                                   # bit 7 in at least a quarter of the bytes
        assert bank[..., [0, 1, 254, 255]].all()                              # every page: non-zero at offsets 0, 1, 254, 255
        assert all(np.unique(bank[i] >> b & 1).size == 2 for i in range(4) for b in range(8))
        assert len({bank[i].tobytes() for i in range(4)}) == 4
    # the recorded DHGR screens carry no byte with bit 7 (the ingests never set it); HGR's do
    g = golden.g4_bitmap_ops
    assert max(int(g["DHGR_%s_%s" % (k, b)].max()) for k in ("src", "tgt") for b in ("main", "aux")) == 127
    assert all(int(g["HGR_%s_main" % k].max()) == 255 for k in ("src", "tgt"))
    for mode in (M.HGR, M.DHGR):
        m, a = M.edge_feeding_screens(mode)
        assert m.dtype == a.dtype == np.uint8 and m.shape == a.shape == (32, 256)
        b = M.body(mode, m, a)
        # neighbouring columns hand each other different headers and different footers, and agree in every other body bit
        assert (M.make_header(mode, b[:, 1:]) != M.make_header(mode, b[:, :-1])).all()
        assert (M.make_footer(mode, b[:, 1:]) != M.make_footer(mode, b[:, :-1])).all()
        feeding = (0x7 << 17 | 1 << 11 | 1 << 10 | 3 << 3) if mode == M.HGR else (7 << 28 | 7 << 3)
        assert not ((b[:, 1:] ^ b[:, :-1]) & np.uint64(~feeding & (1 << 40) - 1)).any()


@pytest.mark.parametrize("mode,name", MODES)
def test_model_equals_the_recorded_vectors(golden, oracle_tables, mode, name):
    g = golden.g4_bitmap_ops
    tab = oracle_tables.get(mode)
    for k in ("src", "tgt"):
        assert np.array_equal(M.pack(mode, g["%s_%s_main" % (name, k)], g["%s_%s_aux" % (name, k)]), g["%s_%s_packed" % (name, k)])
    both = M.pack(mode, np.stack([g[name + "_src_main"], g[name + "_tgt_main"]]), np.stack([g[name + "_src_aux"], g[name + "_tgt_aux"]]))
    assert np.array_equal(both, np.stack([g[name + "_src_packed"], g[name + "_tgt_packed"]]))          # leading dimensions
    sp, tp = g[name + "_src_packed"], g[name + "_tgt_packed"]
    for ia in _banks(mode):
        dw = M.diff_weights(mode, tab, sp, tp, ia)
        assert dw.dtype == np.int32 and np.array_equal(dw, g["%s_dw_%d" % (name, ia)])
        pages, cs = g["%s_delta_pages_%d" % (name, ia)], g["%s_delta_contents_%d" % (name, ia)]
        assert np.array_equal(M.compute_delta_pages(mode, tab, tp, pages, cs, dw[pages], ia), g["%s_delta_%d" % (name, ia)])


@pytest.mark.parametrize("mode,name", MODES)
def test_model_equals_the_oracle_on_all_bit_screens(O, oracle_tables, screens, mode, name):
    main, aux = screens
    tab = oracle_tables.get(mode)
    packed = M.pack(mode, main, aux)
    for i in range(4):
        assert np.array_equal(packed[i], O.pack(mode, main[i], aux[i]))
        assert np.array_equal(packed[i], M.pack(mode, main[i], aux[i]))
    for ia in _banks(mode):
        dw = M.diff_weights(mode, tab, packed[:2], packed[2:], ia)
        for i in range(2):
            assert np.array_equal(dw[i], O.diff_weights(mode, tab, packed[i], packed[2 + i], ia))
    em, ea = M.edge_feeding_screens(mode)
    assert np.array_equal(M.pack(mode, em, ea), O.pack(mode, em, ea))


@pytest.mark.parametrize("mode,name", MODES)
def test_model_equals_the_oracle_for_every_page_and_content(O, oracle_tables, screens, mode, name):
    """all 32 x 256 (page, content) pairs of one screen per mode and bank, the subtrahend random"""
    main, aux = screens
    tab = oracle_tables.get(mode)
    rng = np.random.default_rng(43)
    for ia in _banks(mode):
        packed = M.pack(mode, main[ia], aux[ia])
        rows = rng.integers(-70000, 70001, (32, 256)).astype(np.int32)
        pages, contents = np.divmod(np.arange(8192), 256)
        got = M.compute_delta_pages(mode, tab, packed, pages, contents, rows[pages], ia).reshape(32, 256, 256)
        for p in range(32):
            for c in range(256):
                assert np.array_equal(got[p, c], O.compute_delta_page(mode, tab, packed, p, c, rows[p], ia)), (p, c, ia)
    em, ea = M.edge_feeding_screens(mode)
    packed = M.pack(mode, em, ea)
    zero = np.zeros(256, np.int32)
    for ia in _banks(mode):
        for p in (0, 31):
            for c in (0, 0x7f, 0x80, 0xff, 0x55):
                assert np.array_equal(M.compute_delta_page(mode, tab, packed, p, c, zero, ia), O.compute_delta_page(mode, tab, packed, p, c, zero, ia))


@pytest.mark.parametrize("mode,name", MODES)
def test_every_recorded_apply_step(O, golden, mode, name):
    """after each of the 400 recorded stores the packing is the packing of the memory after that store: model == oracle ==
    pack(memory), and the end state is the recorded one"""
    g = golden.g4_bitmap_ops
    main, aux = g[name + "_src_main"].copy(), g[name + "_src_aux"].copy()
    packed = M.pack(mode, main, aux)
    o_packed, o_main, o_aux = packed.copy(), main.copy(), aux.copy()
    L = O.lib()
    for p, o, ia, val in g[name + "_apply_seq"].tolist():
        M.apply(mode, packed, main, aux, p, o, ia, val)
        L.orc_apply(mode, O._p(o_packed, C.c_uint64), O._p(o_main, C.c_uint8), O._p(o_aux, C.c_uint8), p, o, ia, val)
        assert np.array_equal(packed, o_packed) and np.array_equal(main, o_main) and np.array_equal(aux, o_aux)
        assert np.array_equal(packed, M.pack(mode, main, aux))
    assert np.array_equal(packed, g[name + "_apply_packed"]) and np.array_equal(main, g[name + "_apply_main"])
    if mode == M.DHGR:
        assert np.array_equal(aux, g[name + "_apply_aux"])


def test_the_fix_up_wraps_and_stays_outside_the_window():
    """what the model does literally and the kernel skips: the row-wide rebuild reaches column 127 from column 0 (and back),
    and for every byte offset leaves the byte's own window alone"""
    rng = np.random.default_rng(47)
    for mode in (M.HGR, M.DHGR):
        top = M.HEADER_BITS[mode] + M.BODY_BITS[mode] + M.FOOTER_BITS[mode]
        row = rng.integers(0, 1 << top, 128, dtype=np.uint64)
        last = M.NUM_OFFSETS[mode] - 1
        assert M.fix_neighbours(mode, row, 0)[127] >> np.uint64(top - 3) == M.make_footer(mode, row[0]) >> np.uint64(top - 3)
        assert M.fix_neighbours(mode, row, last)[0] & np.uint64(7) == M.make_header(mode, row[127])
        for o in range(M.NUM_OFFSETS[mode]):
            assert np.array_equal(M.window(mode, M.fix_neighbours(mode, row, o), o), M.window(mode, row, o))
            if 0 < o < last:
                assert np.array_equal(M.fix_neighbours(mode, row, o), row)
