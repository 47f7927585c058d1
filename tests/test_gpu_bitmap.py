"""GPU: screen.Bitmap kernels (P2) through the C ABI against reference-generated vectors."""

import numpy as np
import pytest

from device_guards import ok

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode,name", [(0, "HGR"), (1, "DHGR")])
def test_pack(native, golden, mode, name):
    g = golden.g4_bitmap_ops
    for k in ("src", "tgt"):
        got = native.pack(mode, g["%s_%s_main" % (name, k)], g["%s_%s_aux" % (name, k)])
        assert (got == g["%s_%s_packed" % (name, k)]).all()


@pytest.mark.parametrize("mode", [0, 1])
def test_pack_edges_and_batch(native, O, mode):
    """Empty screen, all-ones screen, and a ragged batch (n=3) against the oracle."""
    rng = np.random.default_rng(5)
    hi = 128 if mode == 1 else 256
    mains = np.stack([np.zeros((32, 256), np.uint8), np.full((32, 256), hi - 1, np.uint8),
                      rng.integers(0, hi, (32, 256), dtype=np.uint8)])
    auxs = mains[::-1].copy()
    got = native.pack(mode, mains, auxs)
    for i in range(3):
        assert (got[i] == O.pack(mode, mains[i], auxs[i])).all()
    blank = np.zeros((32, 256), np.uint8)
    assert (native.pack(mode, blank, blank) == 0).all()


@pytest.mark.parametrize("mode,name", [(0, "HGR"), (1, "DHGR")])
def test_diff_weights_and_delta_pages(native, golden, device_tables, mode, name):
    g = golden.g4_bitmap_ops
    t, _ = device_tables.get(mode)
    sp, tp = g[name + "_src_packed"], g[name + "_tgt_packed"]
    for ia in ((0, 1) if mode == 1 else (0,)):
        dw = native.diff_weights(mode, t, sp, tp, ia)
        assert dw.dtype == np.int32 and (dw == g["%s_dw_%d" % (name, ia)]).all()
        pages = g["%s_delta_pages_%d" % (name, ia)]
        cs = g["%s_delta_contents_%d" % (name, ia)]
        got = native.compute_delta_pages(mode, t, tp, pages, cs, dw[pages], ia)
        assert (got == g["%s_delta_%d" % (name, ia)]).all()


def test_diff_weights_identity_is_zero(native, device_tables):
    rng = np.random.default_rng(8)
    m = rng.integers(0, 128, (32, 256), dtype=np.uint8)
    a = rng.integers(0, 128, (32, 256), dtype=np.uint8)
    p = native.pack(1, m, a)
    t, _ = device_tables.get(1)
    for ia in (0, 1):
        assert (native.diff_weights(1, t, p, p, ia) == 0).all()


# ---- the three kernels against tests/bitmap_model.py: batches, bit 7, page edges, alignments, refusals ---------------------
# (the model itself is held to the recordings and the oracle on the CPU: tests/test_bitmap_model.py)

import ctypes as C                                   # noqa: E402

import bitmap_model as M                             # noqa: E402

GUARD, GUARD64, GUARD32 = 0xA5, 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
MODES = [0, 1]


def _banks(mode):
    return (0, 1) if mode == 1 else (0,)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def _bytes_at(a, lead, trail=5):
    """(buffer, view): the bytes of `a` `lead` bytes into a GUARD-filled device buffer"""
    import torch
    buf = torch.full((lead + a.size + trail,), GUARD, dtype=torch.uint8, device="cuda")
    view = buf[lead:lead + a.size]
    view.copy_(_dev(a.reshape(-1)))
    return buf, view


def _guarded_words(n, dtype, lead=3, trail=4):
    """(buffer, view) of n words of GUARD64 / GUARD32 with `lead` words before and `trail` after"""
    import torch
    buf = torch.full((lead + n + trail,), GUARD64 if dtype == torch.int64 else GUARD32, dtype=dtype, device="cuda")
    return buf, buf[lead:lead + n]


def _guards_kept(buf, view, lead=3):
    import torch
    fill = GUARD64 if buf.dtype == torch.int64 else GUARD32
    b = buf.cpu().numpy()
    return bool((b[:lead] == fill).all() and (b[lead + view.numel():] == fill).all())


@pytest.fixture(scope="module")
def screens():
    """33 + 33 all-bit screens, every one different (bitmap_model.random_screens; its conditions are asserted on the CPU)"""
    main, aux = M.random_screens(61, 33)
    assert len({s.tobytes() for s in main}) == 33 and (main >= 128).mean() > 0.25 and (aux >= 128).mean() > 0.25
    return main, aux


@pytest.fixture(scope="module")
def packed(screens):
    """the model's packing of the screens, per mode: computed once; no test writes to it"""
    return {mode: M.pack(mode, *screens) for mode in MODES}


@pytest.mark.parametrize("n", [1, 2, 5, 33])
@pytest.mark.parametrize("mode", MODES)
def test_pack_batches_equal_the_model_and_their_single_calls(native, screens, packed, mode, n):
    main, aux = screens[0][:n], screens[1][:n]
    got = native.pack(mode, main, aux)
    assert got.shape == (n, 32, 128) and got.dtype == np.uint64
    assert np.array_equal(got, packed[mode][:n])
    for i in sorted({0, n // 2, n - 1}):                 # a screen of a batch depends on nothing but itself
        assert np.array_equal(native.pack(mode, main[i], aux[i]), got[i])
    if n == 5:                                           # ... wherever it stands: the same screens in another order
        order = [3, 0, 4, 1, 2]
        assert np.array_equal(native.pack(mode, main[order], aux[order]), got[order])


@pytest.mark.parametrize("lead_main,lead_aux", [(1, 3), (3, 1)])
@pytest.mark.parametrize("mode", MODES)
def test_pack_at_the_least_alignments_in_guarded_buffers(native, screens, packed, mode, lead_main, lead_aux):
    import torch
    n = 2
    main, aux = screens[0][5:5 + n], screens[1][5:5 + n]
    mbuf, mview = _bytes_at(main, lead_main)
    abuf, aview = _bytes_at(aux, lead_aux)
    assert mview.data_ptr() % 4 == lead_main and aview.data_ptr() % 4 == lead_aux          # one byte off, and three
    obuf, oview = _guarded_words(n * 4096, torch.int64)
    ok(native, native.lib().iiv_pack(mode, n, native.dptr(mview), native.dptr(aview), native.dptr(oview), native.stream_ptr()))
    torch.cuda.current_stream().synchronize()
    assert np.array_equal(oview.cpu().numpy().view(np.uint64).reshape(n, 32, 128), packed[mode][5:5 + n])
    assert _guards_kept(obuf, oview)
    assert np.array_equal(mview.cpu().numpy(), main.reshape(-1)) and np.array_equal(aview.cpu().numpy(), aux.reshape(-1))
    assert (mbuf.cpu().numpy()[:lead_main] == GUARD).all() and (abuf.cpu().numpy()[-5:] == GUARD).all()


def test_dhgr_pack_ignores_bit_7_of_every_byte(native, screens, packed):
    main, aux = screens[0][:3], screens[1][:3]
    want = packed[1][:3]
    assert np.array_equal(native.pack(1, main | 0x80, aux | 0x80), want)
    assert np.array_equal(native.pack(1, main & 0x7f, aux & 0x7f), want)
    # one byte of each of the column's four at a time: a mask dropped on any single one shows
    for which in range(4):
        m, a = main & 0x7f, aux & 0x7f
        (a, m)[which & 1][..., (which >> 1)::2] |= 0x80
        assert np.array_equal(native.pack(1, m, a), want), which


def test_hgr_pack_does_not_read_aux(native, screens, packed):
    import torch
    main = _dev(screens[0][:2])
    junk = torch.full((8,), GUARD, dtype=torch.uint8, device="cuda")              # a pointer-sized buffer: 8 bytes, not a screen
    outs = []
    for aux in (None, junk):
        obuf, oview = _guarded_words(2 * 4096, torch.int64)
        ok(native, native.lib().iiv_pack(0, 2, native.dptr(main), native.dptr(aux), native.dptr(oview), native.stream_ptr()))
        torch.cuda.current_stream().synchronize()
        assert _guards_kept(obuf, oview)
        outs.append(oview.cpu().numpy().view(np.uint64).reshape(2, 32, 128))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], packed[0][:2])
    assert (junk.cpu().numpy() == GUARD).all()


@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("mode", MODES)
def test_diff_weights_batches(native, oracle_tables, device_tables, packed, mode, n):
    """screen k of the source against screen k of the target, every pair different, both banks"""
    table, _ = device_tables.get(mode)
    otab = oracle_tables.get(mode)
    src, tgt = packed[mode][:n], packed[mode][10:10 + n]
    for ia in _banks(mode):
        got = native.diff_weights(mode, table, src, tgt, ia)
        assert got.shape == (n, 32, 256) and got.dtype == np.int32
        want = M.diff_weights(mode, otab, src, tgt, ia)
        assert np.array_equal(got, want)
        assert len({w.tobytes() for w in want}) == n
        for i in range(n):
            one = native.diff_weights(mode, table, src[i], tgt[i], ia)
            assert one.shape == (32, 256) and np.array_equal(one, got[i])
    if mode == 1:
        assert not np.array_equal(M.diff_weights(mode, otab, src, tgt, 0), M.diff_weights(mode, otab, src, tgt, 1))


@pytest.mark.parametrize("mode", MODES)
def test_diff_weights_equal_and_unequal_windows_at_the_page_edges(native, oracle_tables, device_tables, screens, mode):
    """one screen: page 0 of the source is the target's (every window equal), page 1 its complement (every window unequal):
    each byte offset meets both at columns 0 and 127; raw call, guarded output"""
    import torch
    table, _ = device_tables.get(mode)
    otab = oracle_tables.get(mode)
    tm, ta = screens[0][20].copy(), screens[1][20].copy()
    sm, sa = screens[0][21].copy(), screens[1][21].copy()
    sm[0], sa[0] = tm[0], ta[0]
    sm[1], sa[1] = ~tm[1], ~ta[1]
    src, tgt = M.pack(mode, sm, sa), M.pack(mode, tm, ta)
    for o in range(M.NUM_OFFSETS[mode]):
        for col in (0, 127):
            assert M.window(mode, src[0, col], o) == M.window(mode, tgt[0, col], o)
            assert M.window(mode, src[1, col], o) != M.window(mode, tgt[1, col], o)
    d_src, d_tgt = _dev(src), _dev(tgt)
    for ia in _banks(mode):
        obuf, oview = _guarded_words(8192, torch.int32)
        ok(native, native.lib().iiv_diff_weights(mode, native.dptr(table), 1, native.dptr(d_src), native.dptr(d_tgt), ia,
                                                  native.dptr(oview), native.stream_ptr()))
        torch.cuda.current_stream().synchronize()
        got = oview.cpu().numpy().reshape(32, 256)
        assert np.array_equal(got, M.diff_weights(mode, otab, src, tgt, ia)) and _guards_kept(obuf, oview)
        assert not got[0].any() and got[1, [0, 1, 254, 255]].all()


def _delta_screens(mode, screens):
    return {"random": (screens[0][30], screens[1][30]), "edge-feeding": M.edge_feeding_screens(mode)}


@pytest.mark.parametrize("which", ["random", "edge-feeding"])
@pytest.mark.parametrize("mode", MODES)
def test_delta_pages_for_every_page_and_content(native, oracle_tables, device_tables, screens, mode, which):
    """all 32 x 256 (page, content) queries in one call per bank, then the same queries shuffled with duplicates; the rows
    subtracted are random (the kernel subtracts, it does not interpret); contents carry junk above bit 7, which
    include/iivision.h says is ignored.  The model stores the content in every column and rebuilds the row's headers and
    footers with wrap-around; the kernel skips that rebuild."""
    table, _ = device_tables.get(mode)
    otab = oracle_tables.get(mode)
    tgt = M.pack(mode, *_delta_screens(mode, screens)[which])
    rng = np.random.default_rng([67, mode])
    pages, contents = (v.astype(np.int32) for v in np.divmod(np.arange(8192), 256))
    for ia in _banks(mode):
        rows = rng.integers(-70000, 70001, (8192, 256)).astype(np.int32)
        want = M.compute_delta_pages(mode, otab, tgt, pages, contents, rows, ia)
        got = native.compute_delta_pages(mode, table, tgt, pages, contents | 0x5a00, rows, ia)
        assert got.shape == (8192, 256) and got.dtype == np.int32
        assert np.array_equal(got, want)
        pick = rng.integers(0, 8192, 8192)                                  # shuffled, with duplicates (about a third repeat)
        assert len(np.unique(pick)) < 8192 and (np.diff(pages[pick]) < 0).any()
        got = native.compute_delta_pages(mode, table, tgt, pages[pick], contents[pick] | 0x5a00, rows[pick], ia)
        assert np.array_equal(got, want[pick])


@pytest.mark.parametrize("mode", MODES)
def test_refusals_write_nothing(native, device_tables, packed, mode):
    """n < 0, each NULL, a bad mode, HGR with is_aux: IIV_ERR_INVALID and not a byte written; n == 0: OK and not a byte
    written.  (No out-of-range page is passed: d_pages cannot be checked by the host -- include/iivision.h.)"""
    import torch
    L, p, st, null = native.lib(), native.dptr, native.stream_ptr(), C.c_void_p(0)
    table, _ = device_tables.get(mode)
    main, aux = _dev(np.full((2, 32, 256), 0x33, np.uint8)), _dev(np.full((2, 32, 256), 0x44, np.uint8))
    src, tgt = _dev(packed[mode][:2]), _dev(packed[mode][2:4])
    pages, contents = _dev(np.array([0, 31], np.int32)), _dev(np.array([1, 255], np.int32))
    rows = _dev(np.zeros((2, 256), np.int32))
    pbuf, pout = _guarded_words(2 * 4096, torch.int64)
    wbuf, wout = _guarded_words(2 * 8192, torch.int32)
    dbuf, dout = _guarded_words(2 * 256, torch.int32)
    ia = 1 if mode == 1 else 0
    refused = [
        L.iiv_pack(mode, -1, p(main), p(aux), p(pout), st),
        L.iiv_pack(mode, 2, null, p(aux), p(pout), st),
        L.iiv_pack(mode, 2, p(main), p(aux), null, st),
        L.iiv_pack(2, 2, p(main), p(aux), p(pout), st),
        L.iiv_pack(-1, 2, p(main), p(aux), p(pout), st),
        L.iiv_diff_weights(mode, p(table), -1, p(src), p(tgt), ia, p(wout), st),
        L.iiv_diff_weights(mode, null, 2, p(src), p(tgt), ia, p(wout), st),
        L.iiv_diff_weights(mode, p(table), 2, null, p(tgt), ia, p(wout), st),
        L.iiv_diff_weights(mode, p(table), 2, p(src), null, ia, p(wout), st),
        L.iiv_diff_weights(mode, p(table), 2, p(src), p(tgt), ia, null, st),
        L.iiv_diff_weights(7, p(table), 2, p(src), p(tgt), ia, p(wout), st),
        L.iiv_compute_delta_pages(mode, p(table), -1, p(tgt), p(pages), p(contents), p(rows), ia, p(dout), st),
        L.iiv_compute_delta_pages(mode, null, 2, p(tgt), p(pages), p(contents), p(rows), ia, p(dout), st),
        L.iiv_compute_delta_pages(mode, p(table), 2, null, p(pages), p(contents), p(rows), ia, p(dout), st),
        L.iiv_compute_delta_pages(mode, p(table), 2, p(tgt), null, p(contents), p(rows), ia, p(dout), st),
        L.iiv_compute_delta_pages(mode, p(table), 2, p(tgt), p(pages), null, p(rows), ia, p(dout), st),
        L.iiv_compute_delta_pages(mode, p(table), 2, p(tgt), p(pages), p(contents), null, ia, p(dout), st),
        L.iiv_compute_delta_pages(mode, p(table), 2, p(tgt), p(pages), p(contents), p(rows), ia, null, st),
        L.iiv_compute_delta_pages(2, p(table), 2, p(tgt), p(pages), p(contents), p(rows), ia, p(dout), st),
    ]
    if mode == 1:
        refused.append(L.iiv_pack(mode, 2, p(main), null, p(pout), st))             # DHGR needs its aux bank
    else:
        refused += [L.iiv_diff_weights(0, p(table), 2, p(src), p(tgt), 1, p(wout), st),          # HGR has no aux bank
                    L.iiv_compute_delta_pages(0, p(table), 2, p(tgt), p(pages), p(contents), p(rows), 1, p(dout), st)]
    assert refused == [native.ERR_INVALID] * len(refused)
    assert L.iiv_pack(mode, 0, p(main), p(aux), p(pout), st) == 0
    assert L.iiv_diff_weights(mode, p(table), 0, p(src), p(tgt), ia, p(wout), st) == 0
    assert L.iiv_compute_delta_pages(mode, p(table), 0, p(tgt), p(pages), p(contents), p(rows), ia, p(dout), st) == 0
    torch.cuda.synchronize()
    assert (pbuf.cpu().numpy() == GUARD64).all() and (wbuf.cpu().numpy() == GUARD32).all() and (dbuf.cpu().numpy() == GUARD32).all()
    assert (main == 0x33).all() and (aux == 0x44).all() and not rows.any()
    assert np.array_equal(src.cpu().numpy().view(np.uint64), packed[mode][:2]) and np.array_equal(tgt.cpu().numpy().view(np.uint64), packed[mode][2:4])
    # and the same arguments, accepted, fill exactly the slices
    ok(native, L.iiv_pack(mode, 2, p(main), p(aux), p(pout), st))
    ok(native, L.iiv_diff_weights(mode, p(table), 2, p(src), p(tgt), ia, p(wout), st))
    ok(native, L.iiv_compute_delta_pages(mode, p(table), 2, p(tgt), p(pages), p(contents), p(rows), ia, p(dout), st))
    torch.cuda.synchronize()
    assert _guards_kept(pbuf, pout) and _guards_kept(wbuf, wout) and _guards_kept(dbuf, dout)
    assert (pout != GUARD64).all() and (wout != GUARD32).all() and (dout != GUARD32).all()


# ---- screen.Bitmap ------------------------------------------------------------------------------------------------------------

EDGE_OFFSETS = (0, 1, 2, 253, 254, 255)


def _bitmap(mode, main, aux):
    import palette
    import screen
    mm, am = screen.MemoryMap(1, main), screen.MemoryMap(1, aux)
    if mode == 1:
        return screen.DHGRBitmap(palette.Palette.NTSC, mm, am), mm, am
    return screen.HGRBitmap(palette.Palette.NTSC, mm), mm, None


def _stores(mode, n, seed):
    """n seeded stores (page, offset, is_aux, value): offsets on the page's edges a third of the time, pages 0 and 31 forced
    in, both banks, values with all 8 bits"""
    rng = np.random.default_rng([71, mode, seed])
    page = rng.integers(0, 32, n)
    page[rng.permutation(n)[:n // 8]] = rng.choice([0, 31], n // 8)
    offset = np.where(rng.random(n) < 1 / 3, rng.choice(EDGE_OFFSETS, n), rng.integers(0, 256, n))
    is_aux = rng.integers(0, 2, n) if mode == 1 else np.zeros(n, np.int64)
    value = rng.integers(0, 256, n)
    seq = np.stack([page, offset, is_aux, value], axis=1)
    return seq


@pytest.mark.parametrize("mode", MODES)
def test_bitmap_packed_is_the_packing_of_its_memory(native, screens, mode):
    """600 stores; after every 50, bm.packed == the model's pack of the memory the Bitmap now has == native.pack of the same"""
    main, aux = screens[0][25].copy(), screens[1][25].copy()
    bm, mm, am = _bitmap(mode, main, aux)
    assert np.array_equal(bm.packed, M.pack(mode, main, aux))
    m_packed, m_main, m_aux = M.pack(mode, main, aux), main.copy(), aux.copy()
    seq = _stores(mode, 600, 0)
    page, offset, is_aux, value = seq.T
    assert {0, 31} <= set(page.tolist()) and set(EDGE_OFFSETS) <= set(offset.tolist()) and (value >= 128).any() and (value < 128).any()
    assert set(is_aux.tolist()) == ({0, 1} if mode == 1 else {0}) and 0.25 < np.isin(offset, EDGE_OFFSETS).mean() < 0.45
    for k, (p, o, ia, val) in enumerate(seq.tolist()):
        bm.apply(p, o, bool(ia), np.uint8(val))
        M.apply(mode, m_packed, m_main, m_aux, p, o, ia, val)
        if (k + 1) % 50 == 0:
            now_main = bm.main_memory.page_offset
            now_aux = bm.aux_memory.page_offset if mode == 1 else aux
            assert np.array_equal(now_main, m_main) and (mode == 0 or np.array_equal(now_aux, m_aux))
            want = M.pack(mode, now_main, now_aux)
            assert np.array_equal(bm.packed, want), k
            assert np.array_equal(m_packed, want), k
            assert np.array_equal(native.pack(mode, now_main, now_aux), want), k


@pytest.mark.parametrize("mode", MODES)
def test_bitmap_lazy_packed_then_apply(native, screens, mode):
    """`packed` not read before the first apply: it is computed from the constructor's bytes, then the store lands in it"""
    main, aux = screens[0][26].copy(), screens[1][26].copy()
    bm, mm, am = _bitmap(mode, main, aux)
    assert bm._packed is None
    m_packed, m_main, m_aux = M.pack(mode, main, aux), main.copy(), aux.copy()
    for p, o, ia, val in _stores(mode, 40, 1).tolist():
        bm.apply(p, o, bool(ia), np.uint8(val))
        M.apply(mode, m_packed, m_main, m_aux, p, o, ia, val)
    assert np.array_equal(bm.packed, m_packed)
    assert np.array_equal(bm.packed, M.pack(mode, bm.main_memory.page_offset, bm.aux_memory.page_offset if mode == 1 else aux))


@pytest.mark.parametrize("mode", MODES)
def test_bitmap_diff_weights_and_delta_page_through_the_class(native, oracle_tables, screens, mode):
    otab = oracle_tables.get(mode)
    src, _, _ = _bitmap(mode, screens[0][27].copy(), screens[1][27].copy())
    tgt, _, _ = _bitmap(mode, screens[0][28].copy(), screens[1][28].copy())
    for ia in _banks(mode):
        dw = tgt.diff_weights(src, bool(ia))
        assert dw.shape == (32, 256) and np.array_equal(dw, M.diff_weights(mode, otab, src.packed, tgt.packed, ia))
        for page, content in ((0, 0xff), (31, 0x80), (7, 0x2a)):
            got = tgt.compute_delta_page(page, content, dw[page], bool(ia))
            assert np.array_equal(got, M.compute_delta_page(mode, otab, tgt.packed, page, content, dw[page], ia))


# ---- the encoder's own packing ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [1, 0])
def test_encoder_packed_state_is_the_packing_of_its_memory(native, device_tables, mode):
    """one stream through the one-wave greedy kernel over Movie-paced frames: STATE_PACKED == the model's pack of
    STATE_MEM_MAIN / STATE_MEM_AUX read at the same point"""
    import stream_batch
    table, store = device_tables.get(mode)
    fm, fa = stream_batch.synth_frames_torch(1, 2, mode == 1, seed=9)
    batch = stream_batch.StreamBatch(mode, table, store, 1, seeds=[(3, 4)], dm=device_tables.dm[(mode, 5)])
    try:
        batch.enc.set_greedy_kernel(True)
        ops, segs = batch.encode_frames(fm, fa, 2)
        batch.enc.check()
        assert len(segs) >= 2 and ops.shape[0] == 1 and ops.numel() > 0
        main = batch.enc.get_state(native.STATE_MEM_MAIN, 0)
        aux = batch.enc.get_state(native.STATE_MEM_AUX, 0) if mode == 1 else np.zeros((32, 256), np.uint8)
        assert main.any()
        got = batch.enc.get_state(native.STATE_PACKED, 0)
        assert np.array_equal(got, M.pack(mode, main, aux))
    finally:
        batch.close()
