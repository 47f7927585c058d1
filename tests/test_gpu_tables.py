"""GPU: make_data_tables kernels (P1) through the C ABI against the oracle and the
golden vectors.  Integer outputs bit-exact; the float CIE2000 matrix within 1e-5
(the tolerance BASELINE.json's north_star states)."""

import hashlib

import numpy as np
import pytest

import encode_harness as H

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pal", [5, 0])
def test_cie2000_matrix(native, O, golden, pal):
    f, i = native.cie2000_matrix(O.PALETTE_RGB[pal])
    fo, io = O.cie2000_matrix(O.PALETTE_RGB[pal])
    assert np.abs(f - fo).max() < 1e-5
    assert (i == io).all()
    assert (i == golden.g5_tables["dm_i_%d" % pal]).all()
    assert np.abs(f - golden.g5_tables["dm_f_%d" % pal]).max() < 1e-5
    # knife edge: black <-> white truncates to 99
    assert i[0, 15] == 99


@pytest.mark.parametrize("mode,name", [(0, "HGR"), (1, "DHGR")])
def test_pixel_strings_all_values(native, golden, mode, name):
    """K1 against the reference's to_dots + colour model for EVERY masked value."""
    g = golden.g2_dots_pixels
    dots, pix = native.pixel_strings(mode)
    assert (dots.cpu().numpy().view(np.uint32) == g[name + "_dots"]).all()
    assert (pix.cpu().numpy() == g[name + "_pixels"]).all()


@pytest.mark.parametrize("mode,name", [(1, "DHGR"), (0, "HGR")])
def test_full_table_bit_exact(native, oracle_tables, device_tables, mode, name):
    """K2: the whole symmetric table (DHGR 4x2^26, HGR 2x2^28 u16) equals the oracle's."""
    t, _ = device_tables.get(mode)
    got = native.table_to_numpy(t)
    exp = oracle_tables.get(mode)
    assert got.shape == exp.shape
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("mode,name,pal", [(1, "DHGR", 5), (0, "HGR", 5), (1, "DHGR", 0), (0, "HGR", 0)])
def test_lower_triangle_file_format(native, golden, dms, mode, name, pal):
    """symmetric=0 reproduces the array the reference stores in its .npz byte for
    byte (sha256 + sum + 10^4 samples recorded by make_golden.py)."""
    g5 = golden.g5_tables
    t = native.table_to_numpy(native.build_table(mode, dms[pal], symmetric=False))
    assert hashlib.sha256(t.tobytes()).digest() == g5["%s_%d_lower_sha256" % (name, pal)].tobytes()
    assert int(t.astype(np.uint64).sum()) == int(g5["%s_%d_lower_sum" % (name, pal)][0])
    o, idx = g5["%s_%d_sample_o" % (name, pal)], g5["%s_%d_sample_idx" % (name, pal)]
    assert (t[o, idx] == g5["%s_%d_sample_val" % (name, pal)]).all()


@pytest.mark.parametrize("mode", [1, 0])
def test_store_table(native, oracle_tables, device_tables, mode):
    """S[o][content][m] == table[o][(poke(m, content) << bits) + m] for every entry."""
    _, s = device_tables.get(mode)
    L = native.lib()
    bits, noff = L.iiv_masked_bits(mode), L.iiv_num_offsets(mode)
    cb = 7 if mode == 1 else 8
    got = native.table_to_numpy(s).reshape(noff, 1 << cb, 1 << bits)
    full = oracle_tables.get(mode)
    m = np.arange(1 << bits, dtype=np.int64)
    for o in range(noff):
        for c in range(1 << cb):
            if mode == 1:
                pm = (m & ~(0x7f << 3)) | ((c & 0x7f) << 3)
            elif o == 0:
                pm = (m & ~(0xff << 3)) | (c << 3)
            else:
                pm = (m & ~(0xff << 3)) | ((((c & 0x7f) << 1) | (c >> 7)) << 3)
            assert np.array_equal(got[o, c], full[o, (pm << bits) + m]), (o, c)


def test_table_symmetry_properties(native, device_tables):
    """Size-independent properties on the device table itself: symmetric, zero diagonal."""
    import torch
    t, _ = device_tables.get(1)
    for o in range(4):
        m = t[o].view(8192, 8192)
        assert bool((m == m.T).all())
        assert int(torch.diagonal(m).abs().sum()) == 0


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("pal", [5, 0])
def test_split_store_table_is_exact(native, device_tables, dms, mode, pal):
    """The split store table the one-wave greedy kernel reads (csrc/iiv_stream.h): the
    min-plus recurrence behind every value is cut in the middle of the colour string, and
    value = min(l0 + r0, l1 + r1) of a left and a right entry.  Expanded with the encoder's
    own index arithmetic it must equal the dense store table for EVERY (offset, content,
    window) -- both modes, both palettes."""
    import torch
    _, dense = device_tables.get(mode, pal)
    left, right, exp = native.build_split_store_table(mode, dms[pal])
    assert bool((exp == dense).all())
    L = native.lib()
    assert left.numel() == L.iiv_split_table_entries(mode, 0) and right.numel() == L.iiv_split_table_entries(mode, 1)
    # the halves are what makes the table small: 0.5 - 0.6 MiB instead of 8 / 16 MiB
    assert 4 * (left.numel() + right.numel()) <= (640 << 10)
    # left = (E[M-1], E[M]) are finite; right component 0 is "no path" (0x3fff) unless the pixels
    # across the cut can be transposed
    l, r = left.cpu().numpy().view(np.uint32), right.cpu().numpy().view(np.uint32)
    assert int((l & 0xffff).max()) <= 2047 and int((l >> 16).max()) <= 2047 and int((r >> 16).max()) <= 2047
    assert set(np.unique(r & 0xffff)) - set(range(2048)) <= {0x3fff}


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("pal", [5, 0])
def test_narrow_store_table_is_exact(native, device_tables, dms, mode, pal):
    """The narrow form the one-wave and team kernels read (csrc/iiv_stream.h): S = L1 + RF from two 2-byte
    tables, RF = min(r1, r0 - s) carrying the path over a transposition across the cut -- no exceptions, no
    third table.  Re-read with the kernels' own offset arithmetic (the wd word's two fields, the bias) it must
    equal the dense store table for EVERY (offset, content, window); the device counts the entries that differ."""
    _, dense = device_tables.get(mode, pal)
    exp, n_bad = native.build_narrow_store_table(mode, dms[pal], dense)
    assert n_bad == 0
    assert bool((exp == dense).all())


@pytest.mark.parametrize("mode", [1, 0])
def test_encoder_falls_back_when_its_tables_disagree(native, device_tables, dms, mode):
    """iiv_encoder_create holds the folded narrow form to the store table it was GIVEN: with a store table that does
    not come from dm (here: one entry moved) the one-wave / team kernels are refused and the dense-table workgroup
    kernel runs -- exactness is checked, not assumed."""
    table, dense = device_tables.get(mode, 5)
    bad = dense.clone()
    bad.view(-1)[12345] += 1
    enc = native.Encoder(mode, table, bad, 1, dm=dms[5])       # (construction under test: a store table that is not dm's)
    for kern in (True, "team", "shared", "plain"):
        with pytest.raises(native.IIVError):
            enc.set_greedy_kernel(kern)
    enc.set_greedy_kernel(False)
    enc.set_greedy_kernel(None)
    # (the joint content choice then scores from the two-component split table: its packed form is built from the narrow one)
    enc.set_content_choice(True)
    import torch
    fm = torch.zeros((1, 1, 32, 256), dtype=torch.uint8, device="cuda")
    fm[0, 0, 3, 5:40] = 0x2a
    ops = enc.encode(fm, fm.clone() if mode == 1 else None, [(0, 0, 1, 12)])
    enc.check()
    assert ops.shape == (1, 12, 6) and int(ops[0, 0, 0]) == 32 + 3
    enc.close()
    enc = native.Encoder(mode, table, dense, 1, dm=dms[5])     # (... and with the one that is)
    enc.set_greedy_kernel(True)
    enc.close()


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("pal", [5, 0])
def test_split_diff_weight_table_is_exact(native, device_tables, dms, mode, pal):
    """The split diff-weight table of the prologue's IIV_DW_SPLIT mode (csrc/iiv_stream.h): the same
    cut applied to Bitmap.diff_weights' table.  Combined with the prologue's own index
    arithmetic it must equal the full symmetric table for EVERY (offset, source window,
    target window): 2.7e8 (DHGR) / 5.4e8 (HGR) entries, compared on the device."""
    table, _ = device_tables.get(mode, pal)
    assert native.check_split_diff_table(mode, dms[pal], table) == 0
    # and the check can fail: against another palette's table many entries differ
    other, _ = device_tables.get(mode, 0 if pal == 5 else 5)
    assert native.check_split_diff_table(mode, dms[pal], other) > 0


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("pal", [5, 0])
def test_diff_weights_as_sums_of_pair_terms_are_exact(native, device_tables, dms, pal, mode):
    """What the prologue evaluates by default (csrc/iiv_tables.hip: dw_piece_kernel): in a sliding-window colour
    string two transpositions never overlap, so the edit-distance recurrence is a SUM of per-pixel terms and a
    distance is five (DHGR) or nine (HGR: over the windows' dots, two lookups per window) lookups of pixel-pair terms.
    The sum, formed by the prologue's own function / index arithmetic, must equal the full symmetric table for EVERY
    (offset, current window, target window): 4 x 2^26 (DHGR) and 2 x 2^28 (HGR) entries, compared on the device; the
    HGR run also compares the two-lookup dots with to_dots for every window.  (Random matrices:
    test_arbitrary_diff_matrices.)"""
    table, _ = device_tables.get(mode, pal)
    assert native.check_diff_weight_pieces(mode, dms[pal], table) == 0
    other, _ = device_tables.get(mode, 0 if pal == 5 else 5)
    assert native.check_diff_weight_pieces(mode, dms[pal], other) > 0     # (the check can fail)


def test_encoder_rejects_values_beyond_its_key_fields(native, device_tables):
    """diff weights and store values are packed into 11-bit fields; a diff matrix
    or a table that exceeds them must be refused at creation instead of reordering opcodes."""
    import torch
    t, s = device_tables.get(1)
    with pytest.raises(native.IIVError):
        native.Encoder(1, t, s, 1, dm=np.full(256, 205, np.int32))    # 205 * 10 dots > 2047
    big = s.clone()
    big.view(-1)[12345] = 2048
    with pytest.raises(native.IIVError):
        native.Encoder(1, t, big, 1, dm=device_tables.dm[(1, 5)])
    bigt = torch.zeros_like(t)
    bigt.view(-1)[777] = 3000
    with pytest.raises(native.IIVError):
        native.Encoder(1, bigt, s, 1)                                   # table mode: the table is scanned too
    native.Encoder(1, t, s, 1, dm=device_tables.dm[(1, 5)]).close()     # (the real ones are fine)


def test_rejects_bad_arguments(native):
    with pytest.raises(native.IIVError):
        native.build_table(1, np.full(256, 500, np.int32))  # 500*10 > 2047
    with pytest.raises(native.IIVError):
        native.build_table(7, np.zeros(256, np.int32))


def test_user_supplied_table_file(native, O, oracle_tables, device_tables, tmp_path, monkeypatch):
    """A table that does not come from iiv_build_table (VERDICT r1 missing #7): a reference-format
    .npz is loaded and mirrored on the device as Bitmap.edit_distances does (screen.py:343-367), the
    store table is derived from it, and an encoder without a diff matrix encodes with it -- here a
    hand-made table (every distance halved) against the oracle given the same table."""
    import torch
    import screen
    import palette
    mode = 1
    full = oracle_tables.get(mode)
    bits = 13
    a, b = np.divmod(np.arange(1 << (2 * bits), dtype=np.int64), 1 << bits)
    lower = np.where(a > b, full, 0).astype(np.uint16)
    t, s = native.load_table(mode, lower)
    dt, ds = device_tables.get(mode)
    assert bool((t == dt).all()) and bool((s == ds).all())
    # the same through the mirror's file path
    custom_lower = (lower // 2).astype(np.uint16)
    custom_full = (full // 2).astype(np.uint16)
    os_dir = tmp_path / "transcoder" / "data"
    os_dir.mkdir(parents=True)
    np.savez(str(os_dir / "DHGR_palette_5_edit_distance.npz"), edit_distance=custom_lower)
    monkeypatch.chdir(tmp_path)
    # (the flag is part of the cache key -- a rebuild cached BEFORE the flag is set must not
    # be what comes back after it, and a missing file is an error that names the path)
    rebuilt = screen.DHGRBitmap.edit_distances(palette.Palette.NTSC)
    assert rebuilt.dm is not None
    monkeypatch.setattr(screen.Bitmap, "LOAD_TABLE_FILES", True)
    with pytest.raises(FileNotFoundError, match="HGR_palette_5_edit_distance.npz"):
        screen.HGRBitmap.edit_distances(palette.Palette.NTSC)
    try:
        tab = screen.DHGRBitmap.edit_distances(palette.Palette.NTSC)
        assert tab.dm is None
        assert np.array_equal(native.table_to_numpy(tab.table), custom_full)
        fr = np.zeros((1, 2, 2, 32, 256), np.uint8)
        rng = np.random.default_rng(3)
        fr[:] = rng.integers(0, 128, fr.shape)
        fr[..., (np.arange(256) & 127) >= 120] = 0
        # dm = None: table gathers + workgroup kernel
        enc = H.make_encoder(native, (tab.table, tab.store, None), mode, dm=False, rng=[(5, 6)], O=O)
        fm, fa = H.device_frames(mode, list(fr))
        sched = [(0, 0, 1, 291), (0, 1, 1, 198), (1, 1, 1, 94), (1, 0, 1, 292)]
        got = enc.encode(fm, fa, sched).cpu().numpy()[0]
        enc.check()
        with pytest.raises(native.IIVError):
            enc.set_greedy_kernel(True)                               # the one-wave kernel needs dm
        v = O.Video(mode, custom_full, seed_py=5, seed_np=6)
        exp = []
        for (f, ia, _, k) in sched:
            v.encode_frame(fr[0, f, 0], fr[0, f, 1], ia)
            exp.append(v.next(k))
        H.check_ops(got, np.concatenate(exp), "table-only encoder")
        enc.close()
    finally:
        screen.DHGRBitmap._edit_distances.cache_clear()


def test_verify_pins_a_users_tables_on_arrival(native, O, dms, tmp_path, capsys):
    """make_data_tables.verify() compares the reference-format files somebody holds
    with the GPU-built tables.  Stand-in for "real" colormath-built files: the DHGR NTSC table built from
    a matrix with three entries moved (the size of the effect another sRGB matrix has: black <-> white
    99 -> 100).  verify() must call the identical file identical, and for the moved one name the first
    differing entry, recover exactly the moved matrix entries from the file's VALUES alone, and confirm
    that a rebuild from the recovered matrix reproduces the file."""
    import make_data_tables
    import palette
    import screen
    d = tmp_path / "data"
    d.mkdir()
    dm = dms[5].copy()
    moved = {(15, 0): 100, (9, 4): 59, (12, 3): int(dm[12, 3]) + 2}
    for (u, v), val in moved.items():
        dm[u, v] = dm[v, u] = val
    t = native.table_to_numpy(native.build_table(1, dm, symmetric=False))
    np.savez(str(d / "DHGR_palette_5_edit_distance.npz"), edit_distance=t)
    same = native.table_to_numpy(native.build_table(1, dms[0], symmetric=False))
    np.savez(str(d / "DHGR_palette_0_edit_distance.npz"), edit_distance=same)
    lines = []
    n_bad = make_data_tables.verify(str(d), out=lines.append)
    text = "\n".join(lines)
    assert n_bad == 1, text
    assert "DHGR_palette_0_edit_distance.npz: IDENTICAL" in text
    assert "HGR_palette_5_edit_distance.npz: missing, skipped" in text
    assert "DHGR_palette_5_edit_distance.npz:" in text and "DIFFER; first at (offset" in text
    for (u, v), val in moved.items():
        assert "implied dm[%d][%d] = %d" % (u, v, val) in text, text
    assert text.count("implied dm[") == len(moved), text
    assert "0 entries still differ" in text
    # the recovery alone, on an untouched table: the build's own matrix comes back, residual 0
    implied, residual = make_data_tables.implied_diff_matrix(screen.DHGRBitmap, same)
    assert residual == 0
    known = implied >= 0
    assert known.sum() >= 200 and (implied[known] == np.maximum(dms[0], dms[0].T)[known]).all()


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_arbitrary_diff_matrices(native, O, mode, seed):
    """Nothing in the table scheme may lean on the two shipped palettes: random symmetric integer diff matrices (a
    user's own palette, make_data_tables.py:55-87) -- small values, large values up to the key fields' limit, many equal
    entries, zeros off the diagonal (the NTSC palette has a pair of identical greys) -- go through the device's table
    build, the split and narrow store tables (exact for every entry, re-read with the kernels' own arithmetic), the
    split diff-weight table, and a short encode in every kernel form against the oracle built from the same matrix."""
    import torch
    rng = np.random.default_rng(500 + seed)
    hi = (110, 12, 60)[seed - 1]
    dm = rng.integers(0, hi, (16, 16), dtype=np.int32)
    if seed == 3:
        # NOT symmetric: make_data_tables.py:81-87 writes (c, d) and (d, c) on every iteration of its double loop, so the
        # lower triangle of the matrix it was given wins; both table builders must do the same
        np.fill_diagonal(dm, 0)
    else:
        dm = np.triu(dm, 1)
        dm = dm + dm.T                               # symmetric, zero diagonal
    dm[3, 9] = dm[9, 3] = 0                          # two "identical" colours
    dm = np.ascontiguousarray(dm.reshape(256).astype(np.int32))
    otab = O.build_table(mode, dm, symmetric=True)
    table = native.build_table(mode, dm, True)
    assert bool((table.cpu().numpy() == otab).all())
    dense = native.build_store_table(mode, dm)
    exp, n_bad = native.build_narrow_store_table(mode, dm, dense)
    assert n_bad == 0 and bool((exp == dense).all())
    assert native.check_split_diff_table(mode, dm, table) == 0
    assert native.check_diff_weight_pieces(mode, dm, table) == 0
    frames = H.synth(mode, 2, 77 + seed, coherent=True)
    fm, fa = H.device_frames(mode, [frames])
    sched = [(0, 0, 300), (1, 1 if mode else 0, 250), (1, 0, 2200)]
    v = O.Video(mode, otab, seed_py=5, seed_np=6)
    exp_ops = []
    for (f, ia, k) in sched:
        v.encode_frame(frames[f, 0], frames[f, 1] if mode else None, ia)
        exp_ops.append(v.next(k))
    exp_ops = np.concatenate(exp_ops)
    for kern, rec in (("team", True), (True, "split"), ("shared", False), (False, True)):
        enc = H.make_encoder(native, (table, dense, dm), mode, dw=rec, kernel=kern, rng=[(5, 6)], O=O)
        got = enc.encode(fm, fa, H.segments(sched)).cpu().numpy()[0]
        enc.check()
        H.check_ops(got, exp_ops, str((mode, seed, kern, rec)))
        enc.close()
