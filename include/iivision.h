/*
 * iivision.h -- C ABI of the MI355X (gfx950) ][-Vision transcode hot path.
 *
 * This is the drop-in boundary: plain C, pointers and sizes only, no torch
 * types.  Pointers named d_* are DEVICE pointers (HBM), everything else is host
 * memory.  `stream` is a hipStream_t passed as void* (NULL = default stream);
 * all kernels are enqueued on it and, unless noted, calls return without
 * synchronising.  Every function returns IIV_OK (0) or a negative error code;
 * iiv_last_error() gives a message for the calling thread's last failure.
 *
 * The reference (KrisKennaway/ii-vision) is pure Python with no FFI of its own,
 * so each entry point cites the reference Python interface it stands behind
 * (paths relative to the reference checkout).  The host-side mirror of those
 * interfaces lives in ii-vision_amd/transcoder/ and binds this file via ctypes
 * (see INTEGRATION.md).
 */
#ifndef IIVISION_H
#define IIVISION_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IIV_OK 0
#define IIV_ERR_INVALID (-1)   /* bad argument                                   */
#define IIV_ERR_HIP (-2)       /* a HIP runtime call failed                      */
#define IIV_ERR_NO_DEVICE (-3) /* no gfx950 device visible                       */
#define IIV_ERR_ASSERT (-4)    /* a reference `assert` would have fired          */
#define IIV_ERR_OVERFLOW (-5)  /* internal capacity exceeded                     */

/* transcoder/video_mode.py:6-8 */
#define IIV_HGR 0
#define IIV_DHGR 1

/* "iivision-gfx950 <version> build <id>"; <id> = a hash of the sources and flags the library was built from
 * (csrc/Makefile: BUILD_ID).  bench.py prints it and quotes committed counter runs (profiles/pmc_latest.json) only when they
 * carry the same id. */
const char *iiv_version(void);
const char *iiv_last_error(void);
int iiv_device_count(void);

/* ---- mode constants (transcoder/screen.py:606-645, 879-919) -------------- */
int iiv_masked_bits(int mode);       /* MASKED_BITS: HGR 14, DHGR 13          */
int iiv_masked_dots(int mode);       /* MASKED_DOTS: HGR 18, DHGR 10          */
int iiv_num_offsets(int mode);       /* len(BYTE_MASKS): HGR 2, DHGR 4        */
size_t iiv_table_entries(int mode);  /* num_offsets * 2^(2*MASKED_BITS)       */
size_t iiv_store_table_entries(int mode); /* num_offsets * 2^content_bits * 2^MASKED_BITS */

/* ==== P1: make_data_tables (transcoder/make_data_tables.py) ================ */

/* compute_diff_matrix (make_data_tables.py:55-70).  rgb = 16 rows x 3 bytes,
 * row i = RGB of the palette colour whose HGRColours value is i
 * (palette.py:37-78).  One f64 HIP thread per colour pair.  out_f = float
 * Delta-E 2000, out_i = int() of it; either may be NULL.  Synchronises. */
int iiv_cie2000_matrix(const uint8_t rgb[48], double out_f[256], int32_t out_i[256], void *stream);

/* The delta-E 2000 of iiv_cie2000_matrix on n caller-supplied CIE Lab pairs (host arrays,
 * n x 3 doubles each; out: n doubles) -- colormath 3.0.0's delta_e_cie2000 with Kl = Kc = Kh = 1
 * (make_data_tables.py:66-68).  Lets published CIEDE2000 test data be run through the very
 * device function the tables are built with.  Synchronises. */
int iiv_delta_e_cie2000(int n, const double *lab1, const double *lab2, double *out, void *stream);

/* to_dots + dots_to_nominal_colour_pixel_values for every masked value
 * (screen.py:743-789, 983-990; colours.py:100-148).
 * d_dots:   [num_offsets][2^bits] u32      (may be NULL)
 * d_pixels: [num_offsets][2^bits][masked_dots] u8, one colour value per byte */
int iiv_pixel_strings(int mode, uint32_t *d_dots, uint8_t *d_pixels, void *stream);

/* compute_edit_distance (make_data_tables.py:111-174) for one mode; dm is the
 * 16x16 int matrix from iiv_cie2000_matrix (substitute costs follow
 * compute_substitute_costs, make_data_tables.py:73-89).
 * d_out: [num_offsets][2^(2*bits)] u16.
 * symmetric != 0: the full symmetric table that Bitmap.edit_distances() returns
 *                 after its load-time mirror (screen.py:343-367);
 * symmetric == 0: lower triangle only (j < i), byte-identical to the array the
 *                 reference stores in its .npz (make_data_tables.py:156-172). */
int iiv_build_table(int mode, const int32_t dm[256], uint16_t *d_out, int symmetric, void *stream);

/* Derived "store" sub-table used by the greedy loop:
 *   S[o][content][m] = table[o][(mask(poke(m, content)) << bits) + m]
 * i.e. every value Bitmap.compute_delta_page / byte_pair_difference
 * (screen.py:383-398, 525-547) can ever look up, densely packed
 * (DHGR 4x128x8192, HGR 2x256x16384 u16). */
int iiv_build_store_table(int mode, const int32_t dm[256], uint16_t *d_out, void *stream);

/* A table that did NOT come from iiv_build_table -- a user's own
 * transcoder/data/<MODE>_palette_<id>_edit_distance.npz (screen.py:347-350), uploaded as the
 * file holds it: iiv_symmetrise_table applies the load-time mirror of Bitmap.edit_distances
 * (screen.py:352-365: new[a][b] = old[a][b] + old[b][a]) in place, and
 * iiv_store_table_from_table derives the store sub-table from the result.  An encoder created
 * from such a pair with dm == NULL gathers its diff weights from the table (IIV_DW_TABLE)
 * and runs the workgroup greedy kernel.  Asynchronous on `stream`. */
int iiv_symmetrise_table(int mode, uint16_t *d_table, void *stream);
int iiv_store_table_from_table(int mode, const uint16_t *d_table, uint16_t *d_store_out, void *stream);

/* ==== P2: screen.Bitmap operations, batched over n independent screens ===== */
/* Memory maps are (32,256) u8 page/offset arrays (screen.MemoryMap,
 * screen.py:101-125); d_aux is ignored (may be NULL) for HGR. */

/* Bitmap._pack (screen.py:207-226): d_packed [n][32][128] u64.  d_main / d_aux [n][32][256] u8
 * are read byte by byte and need no alignment; DHGR ignores bit 7 of every byte.  n == 0
 * succeeds and writes nothing. */
int iiv_pack(int mode, int n, const uint8_t *d_main, const uint8_t *d_aux, uint64_t *d_packed,
             void *stream);

/* Bitmap.diff_weights (screen.py:400-449) from packed source/target, [n][32][128] u64
 * each, screen k of the one against screen k of the other: d_out [n][32][256] i32. */
int iiv_diff_weights(int mode, const uint16_t *d_table, int n, const uint64_t *d_src_packed,
                     const uint64_t *d_tgt_packed, int is_aux, int32_t *d_out, void *stream);

/* Bitmap.compute_delta_page (screen.py:525-547) for n (page, content) queries
 * against ONE target bitmap: d_pages[n], d_contents[n] i32, d_dw_rows [n][256]
 * i32 (the diff_weights row of each query's page), d_out [n][256] i32.
 * Precondition: every d_pages[q] is in 0..31.  The array lives on the device, so the
 * host cannot check it; any other value reads outside d_tgt_packed.
 * d_contents[q]: the byte is its low 8 bits (content & 0xff); bits 8..31 are ignored.
 * d_dw_rows is only subtracted (out = new weight - d_dw_rows), never interpreted: any
 * i32 rows may be passed, and queries may repeat a page or come in any order. */
int iiv_compute_delta_pages(int mode, const uint16_t *d_table, int n, const uint64_t *d_tgt_packed,
                            const int32_t *d_pages, const int32_t *d_contents,
                            const int32_t *d_dw_rows, int is_aux, int32_t *d_out, void *stream);

/* ==== P3: video.Video (transcoder/video.py:16-301) ========================= */

typedef struct iiv_encoder iiv_encoder;

/* The store table split in two halves whose (content, row) slices are 1-2 KiB (see
 * csrc/iiv_stream.h): value = min(l0 + r0, l1 + r1) of a LEFT and a RIGHT entry, the two
 * halves of the min-plus recurrence behind every table value (make_data_tables.py:92-108).
 * It is what the one-wave greedy kernel reads; iiv_encoder_create builds its own copy.
 * d_left / d_right: iiv_split_table_entries(mode, 0 / 1) u32 each, may be NULL;
 * d_expanded (may be NULL): the dense table rebuilt from the halves with the encoder's own
 * index arithmetic, [iiv_store_table_entries] u16 -- equal to iiv_build_store_table's output,
 * entry for entry (tests).  Synchronises. */
int iiv_build_split_store_table(int mode, const int32_t dm[256], uint32_t *d_left, uint32_t *d_right,
                                uint16_t *d_expanded, void *stream);
size_t iiv_split_table_entries(int mode, int right_half);

/* The form of the split store table the one-wave and the team greedy kernel actually read
 * (csrc/iiv_stream.h, "narrow form"): two 2-byte tables with S = L1 + RF, L1 = l1 and
 * RF = min(r1, r0 - s) + bias, s = the substitution cost of the last pixel left of the cut -- the
 * path over a transposition across the cut folded into the right half, exact for every (offset,
 * content, window) (no exception masks, no dense copy).  This call builds that form from dm and
 * writes every value, obtained with the kernels' own index arithmetic, to d_expanded (same layout as
 * d_store_table); *n_mismatch = entries that differ from d_store_table (0 for a store table built
 * from the same dm: tests).  iiv_encoder_create makes the same comparison with the store table it
 * is given, and an encoder whose tables disagree runs the dense-table workgroup kernel only. */
int iiv_build_narrow_store_table(int mode, const int32_t dm[256], const uint16_t *d_store_table, uint16_t *d_expanded,
                                 unsigned long long *n_mismatch, void *stream);

/* Bitmap.diff_weights' table (screen.py:343-367, 436-443) cut the same way: a diff weight is
 * min(l0 + r0, l1 + r1) of DWL[o][left row of source][left row of target] and
 * DWR[o][right row of source][right row of target] (5 MiB DHGR / 4 MiB HGR instead of
 * 512 MiB / 1 GiB).  iiv_check_split_diff_table builds the halves from dm and compares their
 * combination with EVERY entry of d_table (iiv_build_table(..., symmetric = 1)); *mismatches
 * receives the number of differing entries. */
int iiv_check_split_diff_table(int mode, const int32_t dm[256], const uint16_t *d_table,
                               unsigned long long *mismatches, void *stream);

/* What the prologue's default diff-weight mode (IIV_DW_RECURRENCE) evaluates: for the colour strings of
 * this machine -- sliding 4-dot windows, in which two transpositions can never overlap -- the edit-distance
 * recurrence of make_data_tables.py:92-108 is a plain SUM of per-pixel terms, each a function of two adjacent
 * pixels of both strings, so one distance is five (DHGR, 10 pixels) or nine (HGR, 18 pixels) lookups of
 * pixel-pair terms (6 + 6 dots each) in a 16 KiB table held in LDS (csrc/iiv_tables.hip: dw_piece_kernel).  An HGR
 * window is first turned into its 21 dots (HGRBitmap.to_dots, screen.py:743-789) by two 128/256-entry lookups
 * (csrc/iiv_edit.h: hgr_dot_slot_lo).  This call builds the tables from dm and compares the sum, formed as the
 * prologue forms it, with EVERY entry of d_table (iiv_build_table(..., symmetric = 1): 4 x 2^26 entries DHGR,
 * 2 x 2^28 HGR; HGR also: the two-lookup dots against to_dots for every window); *mismatches receives the number of
 * differing entries. */
int iiv_check_diff_weight_pieces(int mode, const int32_t dm[256], const uint16_t *d_table,
                                 unsigned long long *mismatches, void *stream);

/* One encoder = n_streams independent Video objects of one (mode, palette),
 * all state resident in HBM.  d_table = full symmetric table (iiv_build_table),
 * d_store_table = iiv_build_store_table output; both must outlive the encoder.
 * dm = the 16x16 int CIE2000 matrix the tables were built from, or NULL.
 *   dm != NULL (default mode IIV_DW_RECURRENCE): Bitmap.diff_weights values are
 *     recomputed on the fly with the same recurrence that built the table, or
 *     (IIV_DW_SPLIT) combined from the two halves of a split diff-weight table built
 *     from dm (two gathers per byte from 2.5-4 MiB: measured slower, 1.03 against
 *     0.62 ms per 12288 streams, kept as a third independent way to the same values)
 *     -- both bit-identical, no HBM table traffic; d_table may then be NULL.  The split
 *     store table of the one-wave greedy kernel is built from dm as well.
 *   dm == NULL (IIV_DW_TABLE): they are gathered from d_table (screen.py:436-443);
 *     only the workgroup greedy kernel (which reads d_store_table) is available.
 * Every table value, and max(dm) * MASKED_DOTS, must be <= 2047 (the kernels pack diff
 * weights and store values into 11-bit fields): IIV_ERR_INVALID otherwise.
 * Initial state = Video.__init__ (video.py:21-62): blank screen, zero
 * priorities; both RNG streams seeded as random.seed(0) / np.random.seed(0)
 * until set with iiv_encoder_set_state.
 * Threading / streams: ONE host thread and ONE hipStream_t per encoder.  The launch descriptors of
 * iiv_encode / iiv_encode_streams live in a single device buffer per encoder that is safe only by
 * stream order, so two asynchronous calls on different streams may overwrite descriptors the first
 * call's kernels still read; iiv_encoder_set_option and the iiv_encoder_get_* / set_* state calls use
 * the default stream and synchronise the device.  Different encoders are independent of each other
 * (as different movie.Movie processes are in the reference). */
int iiv_encoder_create(int mode, const uint16_t *d_table, const uint16_t *d_store_table,
                       const int32_t dm[256], int n_streams, iiv_encoder **out);
void iiv_encoder_destroy(iiv_encoder *enc);

#define IIV_OPT_DIFF_WEIGHTS 1 /* how the prologue obtains Bitmap.diff_weights */
#define IIV_DW_TABLE 0         /*   gather from the precomputed table           */
#define IIV_DW_RECURRENCE 1    /*   run the edit-distance recurrence            */
#define IIV_DW_SPLIT 2         /*   combine the two halves of the split table   */
#define IIV_OPT_GREEDY_KERNEL 2 /* shape of the greedy-selection kernel         */
#define IIV_GREEDY_WAVE 0       /*   one 64-lane wave per stream, split store table */
#define IIV_GREEDY_WORKGROUP 1  /*   one 256-thread workgroup per stream, dense store table */
#define IIV_GREEDY_AUTO 2       /*   default: TEAM up to 768 streams, WAVE beyond (dm given at creation; HGR: see WAVE_SHARED) */
#define IIV_GREEDY_TEAM 3       /*   eight waves per stream score the next list entries concurrently and
                                 *   commit in order: the lowest latency for one or a few clips */
#define IIV_GREEDY_WAVE_SHARED 4 /*   WAVE in its LDS-shared form wherever it applies: persistent workgroups whose waves take streams
                                 *   off a queue and share a part of the narrow split store table in LDS -- DHGR: eight streams,
                                 *   both L1 halves of their bank (four of a step's eight table loads become ds_read_u16; needs
                                 *   every stream of a launch on the same bank); HGR: sixteen streams, the even bytes' L1 half
                                 *   (two of eight).  Same output.  WAVE / AUTO choose between this form and the plain one
                                 *   themselves, by what the kernels report about the input: batches that fill the GPU (>= 2048
                                 *   DHGR / 4096 HGR streams) run the shared form unless the nonces decide more than 85 % (DHGR) /
                                 *   30 % (HGR) of the steps (picture-like input: the plain form's 28 waves per CU hide the
                                 *   exact-nonce path better) or the streams emit fewer than 96 real opcodes per launch; until the first report
                                 *   HGR starts shared, DHGR plain (iiv_encoder_input_stats).  This value forces the form */
#define IIV_GREEDY_WAVE_PLAIN 5  /*   WAVE with every table load from the L1 / L2, never the LDS-shared form */
#define IIV_OPT_PREFIX_SORT 3    /* 1 (default): when a generator's opcode budget B is known
                                 * (another restart follows in the same iiv_encode call) and
                                 * 3B <= 2048, only that many highest priorities are ordered;
                                 * 0: always order the whole list.  Same output either way. */
#define IIV_OPT_GREEDY_LDS_PAD 5 /* tuning: extra LDS bytes per stream of the one-wave greedy kernel
                                  * (default 0), which caps how many streams are resident per CU:
                                  * a batch whose size is a whole multiple of the resident streams
                                  * finishes its launches without a half-empty last round */
#define IIV_OPT_CONTENT_CHOICE 6 /* which byte value a greedy step stores */
#define IIV_CONTENT_TARGET 0     /*   default, the reference: the primary location's target byte (video.py:134) */
#define IIV_CONTENT_JOINT 1      /*   NOT reference behaviour -- the "global optimization" the reference's
                                  *   README.md:212-215 leaves as future work: the value c maximising
                                  *     R(c) = (dw[primary] - nd_c[primary]) - (d1 + d2),
                                  *   nd_c[y] = error of byte y of the page once it holds c, d1/d2 = the two
                                  *   smallest negative nd_c[y] - dw[y] over the page's other bytes with non-zero
                                  *   priority (what _compute_error would hand out); ties: the target byte, then
                                  *   the smallest c.  update_priority[primary] becomes nd_c[primary] instead of 0
                                  *   (video.py:140); everything else is the reference's step applied to c.
                                  *   R(target byte) is what the reference's step removes by its own accounting (stores are
                                  *   scored against the target's neighbours, screen.py:542-545), so a joint step never
                                  *   removes less by that accounting; measured on the screen itself a single step may, a
                                  *   frame of them does not (tests/test_gpu_joint.py).  128 / 256 times the lookups of a reference step; runs in the
                                  *   workgroup greedy kernel whatever IIV_OPT_GREEDY_KERNEL says, two byte values per
                                  *   instruction (packed 16-bit sums of the narrow split table). */
#define IIV_CONTENT_JOINT_SPLIT 2 /*  the same choice, byte for byte, computed one byte value at a time from the two-component
                                  *   split table: the slower, independent second implementation (what IIV_CONTENT_JOINT
                                  *   falls back to when the store table given is not the one dm yields). */
#define IIV_OPT_FOURTH_OFFSET 7  /* 0 (default, the reference) / 1: a real fourth offset per opcode.  NOT reference behaviour.
                                  * The player stores every opcode's content byte at FOUR offsets, and video.py:146 says
                                  * "Need to find 3 more offsets to fill this opcode", but the loop's exit test
                                  * `if len(offsets) == 3: break` (video.py:180-181) counts the primary: it stops after two
                                  * more, and :184-186 fill the fourth slot with a copy of the first.  With 1 the test reads
                                  * 4: up to three extra offsets, each handled as the reference handles its two (candidate
                                  * order (delta, nonce, offset), one nonce per candidate, priority 0 skipped, re-queued with a
                                  * nonce when the store leaves an error) -- a quarter of the stream's stores is no longer
                                  * spent on a byte that was just written.  Defined by oracle/iiv_oracle.c
                                  * (orc_video_set_fourth_offset), which is pinned against the reference run with that one
                                  * literal changed (tests/golden/g8_fourth_offset.npz).  Runs in the one-wave greedy kernel (both
                                  * forms) and, for few streams, the eight-wave one (IIV_GREEDY_WORKGROUP falls back to the
                                  * one-wave kernel; needs dm at creation).  Together with IIV_CONTENT_JOINT (round 6): the
                                  * joint score of a byte value then takes its THREE smallest deltas, and the step -- in the
                                  * workgroup kernel, the joint choice's home -- hands out three extra offsets. */
#define IIV_OPT_STREAM_ORDER 8   /* 1 (default) / 0: batches of 2048 streams and more launch the one-wave greedy kernel longest
                                  * stream first -- every stream's shader clocks of a launch are recorded, and every fourth
                                  * launch the streams are sorted by them (a launch ends when its slowest stream does: on
                                  * picture-like input streams differ by 2x and the tail of a launch runs three quarters
                                  * empty).  Streams are independent (movie.py:16-54: one Movie per process in the reference):
                                  * the order they are processed in changes no byte of any stream's output. */
int iiv_encoder_set_option(iiv_encoder *enc, int option, int value);

/* The mode and stream count an encoder was created with (what a caller's frame / output buffers must be sized for:
 * iiv_encode reads and writes n_streams streams whatever the caller's tensors hold -- the host bindings validate
 * their arguments against this; the reference's Video has one stream and one mode, video.py:21-36). */
int iiv_encoder_info(iiv_encoder *enc, int *mode, int *n_streams);

/* state items, per stream.  (The priorities are int32 here, as in the reference; the kernels work on a 16-bit copy of them --
 * 65535 = "see the int32 entry" -- which get_state / get_video_state bring into the int32 arrays before they copy and
 * set_state / set_video_state refill afterwards: DESIGN.md 5, StreamState::up16.) */
#define IIV_STATE_MEM_MAIN 0 /* Video.memory_map.page_offset        u8  [32][256] */
#define IIV_STATE_MEM_AUX 1  /* Video.aux_memory_map.page_offset    u8  [32][256] */
#define IIV_STATE_UP_MAIN 2  /* Video.update_priority               i32 [32][256] */
#define IIV_STATE_UP_AUX 3   /* Video.aux_update_priority           i32 [32][256] */
#define IIV_STATE_RNG_PY 4   /* random.getstate()[1]: 624 words + index, u32[625] */
#define IIV_STATE_RNG_NP 5   /* np.random.get_state()[1], [2]:      u32[625]      */
#define IIV_STATE_OUT_OF_WORK 6 /* Video.out_of_work {False,True}   i32[2]        */
#define IIV_STATE_PACKED 7   /* Video.pixelmap.packed (get only)    u64 [32][128] */
#define IIV_STATE_COUNTERS 8 /* get only: u64[4] = draws_py, draws_np, ops, pad_ops */
int iiv_encoder_get_state(iiv_encoder *enc, int stream_index, int what, void *host_buf, size_t bytes);
int iiv_encoder_set_state(iiv_encoder *enc, int stream_index, int what, const void *host_buf, size_t bytes);
/* The small items -- IIV_STATE_OUT_OF_WORK (movie.py:96 resets the flags at every frame), IIV_STATE_RNG_PY, IIV_STATE_RNG_NP -- of one
 * stream, enqueued on `stream` behind the launches already there: no device-wide synchronisation, no blocking copy (the
 * drop-in Video sets the flags once per frame, between two generators).  host_buf is read before the call returns. */
int iiv_encoder_set_state_async(iiv_encoder *enc, int stream_index, int what, const void *host_buf, size_t bytes, void *stream);
/* the same item of n_streams consecutive streams in one upload: host_buf holds n_streams
 * items of bytes_per_stream back to back (e.g. the seeds of every stream of a batch) */
int iiv_encoder_set_state_range(iiv_encoder *enc, int first_stream, int n_streams, int what, const void *host_buf,
                                size_t bytes_per_stream);

/* Everything a video.Video object exposes, in one round trip (one synchronisation, four copies)
 * instead of one call per item: what the drop-in Video needs whenever somebody looks at it. */
typedef struct {
    uint8_t mem_main[32 * 256], mem_aux[32 * 256];   /* memory_map / aux_memory_map .page_offset     */
    int32_t up_main[32 * 256], up_aux[32 * 256];     /* update_priority / aux_update_priority        */
    uint32_t rng_py[625], rng_np[625];               /* as IIV_STATE_RNG_PY / IIV_STATE_RNG_NP       */
    int32_t out_of_work[2];                          /* out_of_work {False, True}                    */
    uint64_t packed[32 * 128];                       /* pixelmap.packed (filled by get, ignored by set) */
} iiv_video_state;
int iiv_encoder_get_video_state(iiv_encoder *enc, int stream_index, iiv_video_state *host_out);
int iiv_encoder_set_video_state(iiv_encoder *enc, int stream_index, const iiv_video_state *host_in);

/* What video.py looks at when a generator starts (video.py:86-91: the screen-hole assert, the
 * "Similarity" print = update_priority.mean()) plus what the caller can observe between two
 * generators without touching the Video (the global random / np.random states, out_of_work): 5 KB
 * in one round trip instead of the 300 KB of iiv_encoder_get_video_state. */
typedef struct iiv_video_brief {
    int64_t priority_sum[2];   /* sum of update_priority, aux_update_priority            */
    int32_t hole_bytes[2];     /* non-zero bytes inside the screen holes, main / aux map */
    int32_t out_of_work[2];
    uint32_t rng_py[625], rng_np[625];
} iiv_video_brief;
int iiv_encoder_get_video_brief(iiv_encoder *enc, int stream_index, iiv_video_brief *host_out);
/* The same, enqueued on `stream` behind the launches already there (an iiv_encode of a generator's opcodes: the brief then
 * describes the state after them): nothing waits; *host_out is complete once the stream has been synchronised
 * (iiv_encoder_check does).  host_out should be pinned memory.
 * Every brief of one encoder is assembled in ONE device staging struct before it is copied out: all (a)synchronous brief
 * calls of an encoder must therefore be enqueued on one stream (stream order then keeps a later brief from overwriting
 * one whose copy is still in flight) -- the same stream its iiv_encode calls use: an encoder is a one-stream object
 * (see iiv_encoder_create). */
int iiv_encoder_get_video_brief_async(iiv_encoder *enc, int stream_index, iiv_video_brief *host_out, void *stream);

/* Copy / restore the complete state of every stream (screen, priorities, live
 * generator, both RNG streams) on the device.  A caller that must not run ahead of
 * its consumer (a lazy generator, video.py:72-93) can snapshot, produce N opcodes in
 * one launch, and -- if only k < N were consumed -- roll back and re-run exactly k:
 * the computation is deterministic. */
int iiv_encoder_snapshot(iiv_encoder *enc, void *stream);
int iiv_encoder_rollback(iiv_encoder *enc, void *stream);
/* The same with two slots (0: the one the calls above use; 1).  The drop-in Video (transcoder/video.py) runs one generator
 * AHEAD of its caller: behind the launch of generator k it enqueues the generator movie.py:139-148 will ask for next -- the
 * other bank of the same frame -- and needs the state in front of generator k (its caller may abandon k half way:
 * video.py:72-93) and the state in front of generator k + 1 (the guess may be wrong) at the same time. */
int iiv_encoder_snapshot_slot(iiv_encoder *enc, int slot, void *stream);
int iiv_encoder_rollback_slot(iiv_encoder *enc, int slot, void *stream);

/* One segment = what movie.py does between two generator creations:
 * `op_seq = video.encode_frame(target, is_aux)` (if restart) followed by n_ops
 * calls of next(op_seq) (movie.py:94-109).  restart == 0 continues the
 * generator created by the previous segment (same target, same bank). */
typedef struct {
    int32_t frame;   /* index into the frame arrays: the target of this segment */
    int32_t is_aux;  /* bank (video.py:79-84); must be 0 for HGR                */
    int32_t restart; /* 1 = new generator (prologue runs on the first next())   */
    int32_t n_ops;   /* number of next() calls                                  */
} iiv_segment;

/* Video.encode_frame / _index_changes / _heapify_priorities / _compute_error
 * (video.py:72-301) for every stream of the encoder, all segments, in stream
 * order on `stream`.
 * d_frames_main / d_frames_aux: [n_streams][n_frames][32][256] u8 target
 *   memory maps (aux may be NULL for HGR).
 * d_ops_out: [n_streams][sum(n_ops)][6] u8 = (page+32, content, o0, o1, o2, o3)
 *   per yielded tuple (video.py:187, 251).
 * A segment with n_ops == 0 has no effect (the generator is lazy).
 * Does not synchronise; iiv_encoder_check() reports asynchronous failures. */
int iiv_encode(iiv_encoder *enc, const uint8_t *d_frames_main, const uint8_t *d_frames_aux,
               int n_frames, const iiv_segment *segments, int n_segments, uint8_t *d_ops_out,
               void *stream);

/* The same for streams that do NOT share a schedule -- clips of different length, frame
 * rate or every_n_video_frames, each with its own movie.Movie clock (movie.py:16-54):
 * stream s runs segments[seg_begin[s] .. seg_begin[s + 1]) (seg_begin has n_streams + 1
 * entries).  The r-th opcode-emitting segments of all streams share a launch; streams with
 * fewer segments idle.  d_ops_out: stream s writes at d_ops_out + s * ops_stride (bytes),
 * which must hold 6 * (its total n_ops) bytes.  After this call the streams' generators
 * differ, so keep using iiv_encode_streams for this encoder. */
int iiv_encode_streams(iiv_encoder *enc, const uint8_t *d_frames_main, const uint8_t *d_frames_aux,
                       int n_frames, const iiv_segment *segments, const int32_t *seg_begin,
                       uint8_t *d_ops_out, size_t ops_stride, void *stream);

/* Live hand-over of ONE stream's opcodes: the reference's caller pulls its opcodes one next() at a time from a lazy
 * generator (video.py:72-93, movie.py:94-109), and a single clip's chain of steps cannot be computed faster than ~0.5 us per
 * opcode -- about what a Python caller takes to consume one.  So instead of waiting for a launch and then handing its
 * opcodes out, a one-stream encoder can let the caller consume opcode i while the kernel works on i + 1:
 * iiv_encode_live is iiv_encode, with every opcode ALSO written -- one aligned 8-byte store -- into a queue in coherent,
 * GPU-mapped host memory: slot j (j = the opcode's index in the call's output, as in d_ops_out) =
 *   byte 0 page + 32, byte 1 content, bytes 2..5 offsets (the six bytes of d_ops_out), bytes 6..7 `tag` (little endian).
 * A slot is valid as soon as it carries the call's tag (1 .. 65535: the caller changes it from call to call; the queue is
 * zeroed at creation, tag 0 is never valid); an aligned 8-byte store arrives whole, so no fence, flag or synchronisation
 * call is involved.  If a launch ends short of its n_ops (one of the reference's asserts fired -- iiv_encoder_check() says
 * which -- or an internal limit) the slot behind its last opcode holds byte 0 = 0xFF with the tag, and later launches of
 * the call write their own end marks: a reader never waits for a slot that will not be written.
 * iiv_encoder_live_queue: the host address and capacity (opcodes per call) of queue `slot` (0 / 1: one for the live
 * generator, one for a generator enqueued ahead), allocated at the first call; one-stream encoders only.
 * iiv_encode_live: IIV_ERR_INVALID -- before anything is launched or any generator bookkeeping changes -- if the
 * encoder's options keep its launches off the eight-wave team kernel (IIV_CONTENT_JOINT*, IIV_GREEDY_WORKGROUP / WAVE*):
 * the caller then uses iiv_encode.  State, d_ops_out and every other effect are exactly iiv_encode's. */
int iiv_encoder_live_queue(iiv_encoder *enc, int slot, uint64_t **host_queue, int *capacity);
int iiv_encode_live(iiv_encoder *enc, const uint8_t *d_frames_main, const uint8_t *d_frames_aux,
                    int n_frames, const iiv_segment *segments, int n_segments, uint8_t *d_ops_out,
                    int slot, uint32_t tag, void *stream);

/* Synchronises `stream` and returns IIV_ERR_ASSERT / IIV_ERR_OVERFLOW if any
 * stream hit one of the reference's asserts (video.py:87,117,124,137,154-155)
 * or an internal capacity limit; *bad_stream (may be NULL) gets its index. */
int iiv_encoder_check(iiv_encoder *enc, int *bad_stream, void *stream);

/* Kernel timing with HIP events recorded on the launch stream.
 * iiv_encoder_profile(enc, 1) starts collecting; iiv_encoder_profile_read
 * synchronises and returns accumulated milliseconds and launch counts for
 * kernel class 0 = prologue (diff/rank), 1 = greedy (select). */
int iiv_encoder_profile(iiv_encoder *enc, int enable);
int iiv_encoder_profile_read(iiv_encoder *enc, double ms[2], int64_t launches[2]);

/* What the encoder's kernels have reported about the input so far, and which form of the one-wave greedy kernel
 * the next call will run because of it.  (Diagnostic; nothing in the output depends on it.)  The one-wave kernel
 * counts the steps whose extra offsets the nonces decided (video.py:290-301: candidates sharing a delta) and the
 * opcodes it emitted; the counters reach the host by an asynchronous copy that is never waited for, so the figures
 * are those of an earlier call.  stats[0] = that share over the latest interval looked at, stats[1] = real (not padding)
 * opcodes per stream and launch over the same interval (both 0 before any report);
 * *form = IIV_GREEDY_WAVE_SHARED or IIV_GREEDY_WAVE_PLAIN: batches that fill the GPU run the LDS-shared form unless
 * the share is above 85 % (DHGR) / 30 % (HGR) (picture-like input: the plain form's 28 waves per CU hide the exact-nonce
 * path's latency better than the shared form's 16; HGR's shared form, MT19937 in registers, pays more for that path) or the streams emit fewer than 96 real opcodes per launch (converging content that is
 * mostly out of work: the shared form's per-workgroup table copy is not repaid).  IIV_OPT_GREEDY_KERNEL = WAVE_SHARED /
 * WAVE_PLAIN overrule it. */
int iiv_encoder_input_stats(iiv_encoder *enc, double stats[2], int *form);
/* Greedy launches since iiv_encoder_profile(enc, 1), by the kernel that ran them: counts[0] = one wave per stream (plain),
 * [1] = its LDS-shared form, [2] = eight waves per stream (team), [3] = one 256-thread workgroup per stream.  (The form is
 * chosen per launch: bench.py reports how many timed launches ran each.) */
int iiv_encoder_launch_forms(iiv_encoder *enc, int64_t counts[4]);

/* ==== f2: byte emission of the opcode stream (".a2m") ====================== */

/* movie.Movie.emit_stream + done (transcoder/movie.py:113-161) with
 * opcodes.Header / tick opcodes / Ack / Terminate (opcodes.py:64-139) for
 * n_streams independent opcode streams at once:
 *   7-byte header (0xff x6, mode); per opcode [addr_hi, addr_lo, content, o0..o3]
 *   with addr = tick_addr[((tick - 4) / 2) * 32 + page - 32]; a 4-byte ACK
 *   [ack_hi, ack_lo, 0x54|0x55, 0xff] whenever the position reaches 2044 mod 2048
 *   (DHGR: the bank flips at each ACK); then Terminate + zero padding to 2 KiB.
 * d_ops   [n_streams][n_ops][6]  as produced by iiv_encode
 * d_ticks [n_streams][n_ops]     speaker duty cycle of each opcode: 4, 6, ... 66
 * tick_addr / ack_addr / terminate_addr: opcode entry points from the player's
 *   symbol table (player/iivision.dbg; opcodes.py:168-217) -- host memory.
 * max_bytes_out: Movie.max_bytes_out, 0 = unlimited.
 * *out_len receives the stream length (same for every stream); with d_out == NULL
 * nothing is written (size query).  Synchronises.  IIV_ERR_INVALID if a tick is not an even
 * number in 4..66 or an opcode's page byte is outside 32..63 (no such player opcode exists). */
int iiv_emit_stream(int mode, int n_streams, long n_ops, const uint8_t *d_ops, const uint8_t *d_ticks,
                    const uint16_t tick_addr[1024], uint16_t ack_addr, uint16_t terminate_addr,
                    long max_bytes_out, uint8_t *d_out, size_t out_stride, size_t *out_len, void *stream);

/* ==== f3: frame ingest =====================================================
 * RGB frames -> memory maps, the step the reference delegates to the external bmp2dhr tool
 * (frame_grabber.py:68-115; README.md:217-221 wishes for a "direct image encoding").  That
 * tool is not part of the reference's source, so there is no reference output to match; the
 * conversion is SPECIFIED here (integer arithmetic only, so every implementation agrees bit
 * for bit -- the test suite's CPU restatement and the HIP kernel do):
 *   - two source pixels (2k, 2k+1 of a 280-pixel row) are averaged, (a + b + 1) / 2 per
 *     channel, into colour pixel k (140 per row); the ordered-dither offset
 *     floor((2 * B[y & 3][k & 3] - 15) * dither / 16), B = the 4x4 Bayer matrix
 *     {0,8,2,10; 12,4,14,6; 3,11,1,9; 15,7,13,5}, is added and the result clamped to 0..255;
 *   - colour distance = 2 dr^2 + 4 dg^2 + 3 db^2, ties to the lower colour value;
 *   - DHGR: the nearest of the 16 palette colours; its value IS the pattern of the pixel's
 *     aligned dot quad (colours.py:100-134: a repeating quad P shows colour value P), dot X of
 *     the row = bit X & 3 of quad X >> 2; dots are packed 7 per byte, aux / main alternating
 *     (screen.py:822-826), bit 7 clear (video.py:137);
 *   - HGR: per screen byte the palette bit (0: black 0, violet 3, green 12, white 15; 1: black,
 *     blue 6, orange 9, white) whose summed nearest-colour error over the byte's seven dots is
 *     smaller (ties to 0), then dot X = bit X & 1 of the 2-dot pattern of pixel X >> 1 under that
 *     palette bit (pattern bit 0 = the even dot column, colours.py:18-44);
 *   - bytes land at y_to_base_addr (screen.py:16-22); screen holes stay 0.
 * dither == IIV_DITHER_DIFFUSION replaces the ordered dither by Floyd-Steinberg error diffusion (the reference calls
 * bmp2dhr with D9, an error-diffusion dither: frame_grabber.py:80-82,106-108; bmp2dhr itself cannot be matched --
 * it is not here).  Over the 140 x 192 colour pixels, rows top to bottom, pixels left to right, per channel:
 *   value = clamp(mean of the two source pixels + floor(acc / 16), 0, 255); e = value - chosen colour;
 *   acc[right] += 7 e, acc[below left] += 3 e, acc[below] += 5 e, acc[below right] += e (sixteenths; targets outside
 *   the picture are dropped).  DHGR: the chosen colour is the nearest of the 16.  HGR: the palette bit of screen byte b
 *   is fixed just before the first pixel whose first dot lies in b is quantised -- for both palette bits the nearest-
 *   colour errors of the pixels whose first dot lies in b are summed (each weighted by the number of its dots in b:
 *   2 or 1), their values taken with the error accumulated up to then; the smaller sum wins, ties to 0 -- and a pixel
 *   takes the nearest of the four colours of the palette bit of the byte holding its first dot; bit 0 / 1 of its
 *   pattern go to its first / second dot.
 * d_rgb: [n_frames][192][280][3] u8 (frame_grabber.py:75,100 resizes every frame to 280x192);
 * palette_rgb: 16 x 3 host bytes, row i = colour value i (palette.py:37-78); dither: amplitude
 * 0..255 of the ordered dither (0 = none), or IIV_DITHER_DIFFUSION; d_main / d_aux: [n_frames][32][256] u8 memory maps (d_aux ignored for
 * HGR).  d_rgb 4-byte aligned, d_main / d_aux 8-byte aligned.  Asynchronous on `stream` (the palette is read before the call
 * returns; nothing is allocated): a batch's frames can be converted while the previous batch is being encoded. */
#define IIV_DITHER_DIFFUSION 256
int iiv_frames_to_memory_maps(int mode, const uint8_t palette_rgb[48], int n_frames, const uint8_t *d_rgb,
                              int dither, uint8_t *d_main, uint8_t *d_aux, void *stream);

/* The error diffusion with a CHOSEN kernel: everything as iiv_frames_to_memory_maps with IIV_DITHER_DIFFUSION -- the
 * averaging of the two source pixels, the colour distance and its ties, DHGR's nearest of the 16, HGR's palette bit of screen
 * byte b fixed just before the first pixel whose first dot lies in b is quantised (for both palette bits the nearest-colour
 * errors of the pixels whose first dot lies in b are summed, each weighted by the number of its dots in b, their values taken
 * with the error accumulated up to then; the smaller sum wins, ties to 0; a pixel takes the nearest of the four colours of
 * the palette bit of the byte holding its first dot), packing, holes, alignments, asynchrony, nothing allocated -- except
 * where a pixel's error goes:
 *   weights[5 * dy + dx + 2], dy = 0..2, dx = -2..+2, is the share, in `divisor`-ths, of pixel (y + dy, k + dx).
 *   Rows top to bottom, pixels left to right, per channel:
 *   value = clamp(mean of the two source pixels + floor(acc / divisor), 0, 255), floor towards minus infinity;
 *   e = value - chosen colour; acc[y + dy][k + dx] += weights[5 * dy + dx + 2] * e; targets outside the 140 x 192 picture
 *   are dropped.
 * IIV_ERR_INVALID before anything is launched, nothing written: a bad mode or alignment; divisor outside 1..64; any of
 * weights[0..2] non-zero (the pixel itself and what lies left of it on its row); a sum of weights above divisor.  (So
 * |acc| <= 255 * 64, and the kernel's floor(acc / divisor) is an exact multiply-and-shift.)  All-zero weights are legal: no
 * diffusion.  {0,0,0,7,0, 0,3,5,1,0, 0,0,0,0,0} / 16 is Floyd-Steinberg and gives the bytes of IIV_DITHER_DIFFUSION, through
 * another kernel (csrc/iiv_diffuse.hip): this entry point never runs iiv_frames_to_memory_maps' own.  The named kernels
 * (Jarvis, Stucki, Atkinson, Burkes, Sierra ...) are a table of the Python layer, transcoder/frame_grabber.py:
 * DIFFUSION_KERNELS.  Its "buckels" -- the D9 the reference asks bmp2dhr for (frame_grabber.py:80-82,106-108) -- is
 * {0,0,0,2,1, 0,1,2,1,0, 0,0,1,0,0} / 8 AS REMEMBERED from bmp2dhr's source, which is not here to check: an assumption, and
 * no equality with bmp2dhr's output is claimed for it or for anything else here. */
int iiv_frames_to_memory_maps_diffused(int mode, const uint8_t palette_rgb[48], int n_frames, const uint8_t *d_rgb,
                                       const uint8_t weights[15], int divisor,
                                       uint8_t *d_main, uint8_t *d_aux, void *stream);

/* The same bytes for a slice of the opcode stream, asynchronously (no host round trip, no
 * synchronisation): opcodes [first_op, first_op + n_ops) of every stream, so that a movie can
 * be emitted while it is being encoded (iiv_encode -> iiv_emit_chunk -> copy to the host).
 * d_ops points at opcode first_op of stream 0, streams ops_stride BYTES apart (d_ticks /
 * ticks_stride likewise, in bytes; d_ticks == NULL: every opcode carries const_tick).
 * d_tick_addr: the 1024 tick opcode addresses in DEVICE memory.  The slice's bytes are the
 * stream positions [*first_byte, *first_byte + *n_bytes) -- the 7-byte header belongs to
 * opcode 0, an ACK to the opcode in front of it -- written at d_out + s * out_stride.
 * Terminate + padding are not written (iiv_emit_stream, or the caller after the last slice).
 * d_out == NULL: only the byte range is computed.  d_err (device int, may be NULL) is set to
 * 1 if a tick is not an even number in 4..66 or a page is outside 32..63. */
int iiv_emit_chunk(int mode, int n_streams, long first_op, long n_ops, const uint8_t *d_ops, size_t ops_stride,
                   const uint8_t *d_ticks, size_t ticks_stride, int const_tick, const uint16_t *d_tick_addr,
                   uint16_t ack_addr, uint8_t *d_out, size_t out_stride, size_t *first_byte, size_t *n_bytes,
                   int *d_err, void *stream);


/* ==== f4: the audio track ===================================================
 * audio.Audio (transcoder/audio.py:9-107) and the tick of movie.Movie.encode (movie.py:67-111): interleaved int16 PCM
 * -> one speaker duty cycle per player opcode.  Per stream: frames are cut into decode blocks of block_frames frames
 * (audio.py:98 read_data(128 * 1024); the last block is short), each block is averaged over its channels
 * (audio.py:51-55, librosa.to_mono) and resampled on its own from rate to bitrate (audio.py:56-58: librosa.resample,
 * res_type='scipy', scale=True: scipy.signal.resample to ceil(n * bitrate / rate) samples, divided by
 * sqrt(bitrate / rate); rate == bitrate: untouched), then a /= 16384, a *= normalization, au = clip(int(a * 16), -15, 16)
 * (audio.py:100-105), tick = 2 au + 34 (movie.py:104-107).  Opcode k of a movie carries tick k.  The arithmetic is fp32
 * FFTs on the device (csrc/iiv_audio.hip).
 * d_pcm: stream s at d_pcm + s * pcm_stride (int16 elements), n_frames[s] frames of channels[s] interleaved samples at
 * rate[s] Hz -- host arrays of n_streams entries.  Streams are independent; at most 65535 per call.
 * Transforms run on at most 2^24 points: a call whose decode block (or, for iiv_audio_resample / _normalization, whole
 * stream / prefix), before or after resampling, is not a power of two and longer than 2^23 points is refused with
 * IIV_ERR_INVALID before anything is launched (e.g. the normalisation of 8 kHz mono longer than about 570 s).
 * Device memory is allocated stream-ordered per call and freed behind the call's work; nothing is kept between calls. */

/* The tick count of one stream (the sum of the blocks' ceil(n * bitrate / rate), each product in float64 as librosa
 * computes it).  Host only, no device; a negative error code for bad arguments. */
long iiv_audio_tick_count(long n_frames, int rate, int bitrate, long block_frames);

/* Audio.audio_stream (audio.py:93-107) for n_streams streams: d_ticks [n_streams][ticks_stride] uint8 receives tick k
 * of stream s at d_ticks + s * ticks_stride + k for k < n_ticks[s] (host, filled before the call returns; may be NULL);
 * bytes past a stream's tick count are not written.  normalization: host, per stream (Audio.normalization, e.g. from
 * iiv_audio_normalization); IIV_ERR_INVALID if one is zero or not finite (16384 / 0 for a silent prefix: the reference
 * turns the resulting NaN into an undefined int).  Asynchronous on `stream`. */
int iiv_audio_ticks(int n_streams, const int16_t *d_pcm, size_t pcm_stride, const long *n_frames, const int *channels,
                    const int *rate, int bitrate, long block_frames, const double *normalization, uint8_t *d_ticks,
                    size_t ticks_stride, long *n_ticks, void *stream);

/* Audio._decode of each whole stream as ONE block (audio.py:47-60): d_out [n_streams][out_stride] float32, sample k of
 * stream s at d_out + s * out_stride + k for k < n_out[s] (host, may be NULL).  What iiv_audio_normalization
 * measures, exposed for tests and tools.  Asynchronous on `stream`. */
int iiv_audio_resample(int n_streams, const int16_t *d_pcm, size_t pcm_stride, const long *n_frames, const int *channels,
                       const int *rate, int bitrate, float *d_out, size_t out_stride, long *n_out, void *stream);

/* Audio._normalization (audio.py:60-78) per stream: the prefix audioread's default read_data() blocks (1024 frames)
 * deliver until more than 10 MiB are held, decoded as one block, norm = max(|percentile(a, [0.5, 99.5])|) (linear
 * interpolation, order statistics selected on the device) -> normalization[s] = 16384 / norm (host; inf for a silent
 * prefix).  Synchronises. */
int iiv_audio_normalization(int n_streams, const int16_t *d_pcm, size_t pcm_stride, const long *n_frames, const int *channels,
                            const int *rate, int bitrate, double *normalization, void *stream);

/* ==== f5: the resize ========================================================
 * frame_grabber.py:75,100 (`_frame.resize((280, 192), resample=Image.LANCZOS)`): every decoded frame is resized to
 * 280x192 before anything else.  Byte-exact with Pillow's Image.resize(..., LANCZOS) of a uint8 RGB image (DESIGN.md 11;
 * pinned against Pillow 12.2.0 -- the reference pins 9.4.0, whose fixed-point core is assumed to be the same):
 *   - per axis (in -> out samples): scale = in / out, filterscale = max(scale, 1), support = 3 filterscale,
 *     ksize = 2 ceil(support) + 1; output xx: center = (xx + 0.5) scale, xmin = max((int)(center - support + 0.5), 0),
 *     count = min((int)(center + support + 0.5), in) - xmin, w[x] = lanczos((x + xmin - center + 0.5) * (1 / filterscale))
 *     for x < count, lanczos(x) = sinc(x) sinc(x / 3) on [-3, 3), all float64 with libm sin; the weights are divided by
 *     their sum (summed in order; when it is non-zero) and rounded to k = (int)(w 2^22 +- 0.5) (the sign of w);
 *   - a pass: out = clamp((2^21 + sum_x pixel[xmin + x] k[x]) >> 22, 0, 255) in int32, each channel on its own;
 *   - (h, w) == (H, W): a copy; one axis changed: one pass; otherwise the horizontal pass first -- the vertical one first
 *     when h > 100 w (the installed Pillow's rule) -- and the uint8 result of the first pass feeds the second.
 * Coefficients are computed on the host; the device only multiplies and adds integers (csrc/iiv_resize.hip). */

/* The coefficient table of one axis (frame_grabber.py:75,100), host only (no device): *ksize receives the taps per
 * output sample; bounds [out_size][2] = (xmin, count), coeffs [out_size][*ksize] fixed-point, zero past count.
 * bounds == coeffs == NULL: only *ksize (size query).  in_size 1..8192, out_size 1..1024, else IIV_ERR_INVALID. */
int iiv_resize_coeffs(int in_size, int out_size, int *ksize, int32_t *bounds, int32_t *coeffs);

/* Resize n frames (frame_grabber.py:75,100): d_src frame f, row y, pixel x, channel c at
 * d_src + f * frame_stride + y * row_stride + 3 x + c (byte strides: a crop, a letterbox cut or a strided view needs no
 * copy; rows and frames must not overlap) -> d_dst [n][H][W][3] contiguous.  1 <= h, w <= 8192, 1 <= H, W <= 1024, else
 * IIV_ERR_INVALID before anything is launched.  No alignment is required.  The coefficient tables are kept per (device,
 * in, out) for the life of the process: the FIRST call with a size pair on a device builds and uploads them synchronously;
 * every later call is asynchronous on `stream` (its scratch is allocated and freed stream-ordered), so d_src and d_dst must
 * stay alive and untouched until `stream` has reached the call. */
int iiv_resize_frames(int n, int h, int w, const uint8_t *d_src, size_t frame_stride, size_t row_stride, int H, int W,
                      uint8_t *d_dst, void *stream);

/* ==== f6: mono playback mode ================================================
 * RGB frames -> memory maps for a MONOCHROME monitor (the reference README's "mono playback mode", not started there).
 * On such a monitor a (D)HGR screen is a W x 192 one-bit picture, W = 560 dots (DHGR) or 280 (HGR), so the source frame
 * has one pixel per dot.  Like f3 the conversion is SPECIFIED here, integer arithmetic only, so every implementation
 * agrees bit for bit (tests/mono_model.py restates it; csrc/iiv_mono.hip computes it):
 *   - luma Y = (77 R + 150 G + 29 B + 128) >> 8 of source pixel (X, y) = dot X of row y;
 *   - ordered dither, amplitude `dither` 0..255: v = clamp(Y + floor((2 * B[y & 3][X & 3] - 15) * dither / 16), 0, 255), B the
 *     4x4 Bayer matrix of f3; dot = v >= 128;
 *   - dither == IIV_DITHER_DIFFUSION: Floyd-Steinberg over the W x 192 dots, rows top to bottom, dots left to right:
 *     v = clamp(Y + floor(acc / 16), 0, 255), dot = v >= 128, e = v - 255 * dot; acc[right] += 7 e, acc[below left] += 3 e,
 *     acc[below] += 5 e, acc[below right] += e (sixteenths; targets outside the picture are dropped); floor is towards
 *     minus infinity, as in f3;
 *   - packing: dot X goes to bit X % 7 of byte X / 7 of the row.  DHGR: even bytes of the row's 80 go to the aux bank and
 *     odd ones to main, column X / 14 (screen.py:822-826).  HGR: the row's 40 bytes go to main (on a mono screen the palette
 *     bit is only a half-dot shift: it stays clear).  Bit 7 is clear in both modes;
 *   - bytes land at y_to_base_addr (screen.py:16-22); the screen holes are written as 0.
 * The cost matrix that goes with it (palette.MonoPalette.diff_matrix(), host) prices a change of colour value a -> b of
 * the sliding-window model -- four dots, bit k the dot at screen position = k mod 4 -- by the dots it changes:
 * dm[a][b] = 16 |popcount(a) - popcount(b)| + 8 popcount(a ^ b); iiv_build_table / iiv_build_store_table /
 * iiv_encoder_create take it as they take any 16 x 16 matrix.
 * d_rgb: [n_frames][192][W][3] u8, 4-byte aligned; d_main / d_aux: [n_frames][32][256] u8 memory maps, 8-byte aligned (d_aux
 * ignored for HGR).  IIV_ERR_INVALID for a bad mode, dither or alignment, before anything is launched.  Asynchronous on
 * `stream`, as iiv_frames_to_memory_maps is: nothing synchronises, the error diffusion's scratch (the frames' luma in the
 * order its lanes read it) is allocated and freed stream-ordered, so d_rgb, d_main and d_aux must stay alive and untouched
 * until `stream` has reached the call. */
int iiv_frames_to_memory_maps_mono(int mode, int n_frames, const uint8_t *d_rgb, int dither, uint8_t *d_main,
                                   uint8_t *d_aux, void *stream);

/* ==== f7: preview ==========================================================
 * Screen memory -> 560 x 192 RGB: what a memory map (an ingest's output, an encoder's screen after any number of opcodes)
 * puts on the screen, through the reference's own colour model (colours.py:100-134, screen.py:743-789, 983-990) -- the model
 * that prices every store, which iiv_pixel_strings evaluates per masked value -- stated per screen row instead of per packed
 * value.  One difference from the reference: a row starts with no dots to its left (the reference's packed form leaks the
 * previous row's last byte into the next row's header, which it marks as a TODO, screen.py:190).  Integer rules only, so
 * every implementation agrees byte for byte (tests/render_model.py restates them and is held to the reference-recorded
 * strings; csrc/iiv_render.hip computes them).  Output is 560 dots by 192 rows in both modes.
 *   Dots of row y.  The 40 bytes of row y are at y_to_base_addr(y) in the memory map (screen.py:16-22).
 *   - DHGR: the byte sequence is aux[0], main[0], aux[1], main[1], ... for 80 bytes.  Dot 7 i + j is bit j of byte i, for
 *     j = 0..6.  Bit 7 is ignored.
 *   - HGR: byte i has palette bit p_i (bit 7) and data bits 0..6.  For dot x, let i = x / 14 and r = x % 14.
 *       If p_i = 0, the dot is bit r / 2.
 *       If p_i = 1 and r > 0, the dot is bit (r - 1) / 2.
 *       If p_i = 1 and r = 0, the dot is bit 6 of byte i - 1, or 0 for i = 0.
 *       The 561st dot, which a shifted last byte would light, is dropped.
 *   Colour of dot x.  Let w = d[x-3] | d[x-2] << 1 | d[x-1] << 2 | d[x] << 3, with dots left of the row taken as 0.  The
 *   colour value is rol4(w, (x + 1) & 3), where rol4 is colours.py:87-97.  Pixel (y, x) is
 *   palette_rgb[3 * value .. 3 * value + 2].  palette_rgb is the same 16 x 3 host array the ingest entry points take.
 *   (So an aligned repeating quad P shows colour value P from dot 3 on: what iiv_frames_to_memory_maps promises.)
 * Screen holes are never read.  In HGR, d_aux is ignored and may be NULL.
 * d_main / d_aux: [n][32][256] u8 memory maps, 8-byte aligned; d_rgb: [n][192][560][3] u8, 16-byte aligned.  Asynchronous on
 * `stream`; the palette is read before the call returns; nothing is allocated.  n == 0 succeeds and writes nothing.
 * IIV_ERR_INVALID before anything is launched: a bad mode, n < 0, a NULL d_main or d_rgb, a NULL d_aux in DHGR, a bad
 * alignment. */
int iiv_render_rgb(int mode, const uint8_t palette_rgb[48], int n, const uint8_t *d_main, const uint8_t *d_aux, uint8_t *d_rgb,
                   void *stream);

/* The same rendering of the encoder's OWN device copy of IIV_STATE_MEM_MAIN / IIV_STATE_MEM_AUX, for streams
 * first_stream .. first_stream + n_streams - 1 -> d_rgb [n_streams][192][560][3]: no host round trip.  Refusals as
 * iiv_render_rgb's, and a stream range that is not inside the encoder's.  It changes nothing in the encoder; ordering
 * against a running encode is by `stream`, as for iiv_encoder_get_video_brief_async (an encoder is a one-stream object). */
int iiv_encoder_render(iiv_encoder *enc, int first_stream, int n_streams, const uint8_t palette_rgb[48], uint8_t *d_rgb,
                       void *stream);

/* ==== f8: screen error ======================================================
 * How far is what the screen shows from a reference picture: exact integer sums of squared differences, per frame, per
 * colour channel, at three block sizes, computed on the device without the rendered picture ever leaving the chip
 * (csrc/iiv_render_error.hip; tests/render_error_model.py restates this section on top of tests/render_model.py).
 *   S[f][y][x][c] is the byte iiv_render_rgb (f7) would write for frame f: 192 rows of 560 dots, 3 channels.
 *   d_ref is [n][192][ref_width][3] u8, ref_width 560 (one reference pixel per dot: what the mono ingest takes) or 280 (one per
 *   two dots: what the colour ingest and the resize deliver): R[f][y][x][c] = ref[f][y][x * ref_width / 560][c].
 *   D = (int)S - (int)R.
 *   d_out is [n][3][3] uint64, [frame][level][channel]:
 *     level 0 (dot):                     sum over y, x of D[y][x]^2
 *     level 1 (quad of four dots: the colour pixel of the 140-wide ingest):
 *                                        sum over y, q < 140 of (D[y][4q] + D[y][4q+1] + D[y][4q+2] + D[y][4q+3])^2
 *     level 2 (unit of sixteen dots):    sum over y, u < 35 of (sum over k < 16 of D[y][16u+k])^2
 *   Levels 1 and 2 are low-passed errors: a dithered picture is meant to be wrong per dot and right on average, and level 0
 *   alone would rank "no dither" first.  Every block lies in one row (there is no vertical low-pass).
 * The call overwrites all 72 bytes of every frame; the caller need not zero d_out.  The sums are integers, so d_out is exact
 * whatever the order of summation; the largest possible per frame are 107 520 * 255^2 (7.0e9), 26 880 * 1020^2 (2.8e10) and
 * 6 720 * 4080^2 (1.1e11, with D = +-255 everywhere): none fits 32 bits.
 * d_main / d_aux: [n][32][256] u8 memory maps, 8-byte aligned, as for f7 (screen holes are never read; d_aux is ignored and
 * may be NULL in HGR); d_ref 16-byte aligned; d_out 8-byte aligned.  Asynchronous on `stream`; the palette is read before
 * the call returns; nothing is allocated.  n == 0 succeeds and writes nothing.  IIV_ERR_INVALID before anything is launched,
 * with nothing written: a bad mode, n < 0, a NULL palette_rgb, d_main, d_ref or d_out, a NULL d_aux in DHGR, ref_width not
 * 280 or 560, a bad alignment. */
int iiv_render_error(int mode, const uint8_t palette_rgb[48], int n, const uint8_t *d_main, const uint8_t *d_aux,
                     const uint8_t *d_ref, int ref_width, uint64_t *d_out, void *stream);

/* The same measurement of the encoder's OWN device copy of the maps, as iiv_encoder_render renders them, for streams
 * first_stream .. first_stream + n_streams - 1: reference picture i of d_ref [n_streams][192][ref_width][3] belongs to
 * stream first_stream + i, d_out is [n_streams][3][3].  Refusals as iiv_render_error's, and a stream range that is not inside
 * the encoder's.  It changes nothing in the encoder; ordering against a running encode is by `stream`. */
int iiv_encoder_render_error(iiv_encoder *enc, int first_stream, int n_streams, const uint8_t palette_rgb[48],
                             const uint8_t *d_ref, int ref_width, uint64_t *d_out, void *stream);

/* ==== f9: reading an opcode stream ==========================================
 * The inverse of f2: a stream as written -- by iiv_emit_stream, by the reference's Movie, by an older build -- is checked,
 * decoded back to the encoder's records, and replayed to the screen memory a player holds after k opcodes, which is what f7
 * and f8 take (csrc/iiv_a2m_read.hip; tests/a2m_model.py restates this section in numpy).
 *   Layout.  L is the stream's length.  Slot k is the 7 bytes at P(k): P(k) = 7 + 7 k for k < 291, and
 *   2048 (1 + (k - 291) / 292) + 7 ((k - 291) % 292) from there on (the position f2 writes opcode k at).  A slot's address is
 *   big-endian in its first two bytes.  T is the 1024-entry tick-address table [(tick - 4) / 2][page - 32].  n_ops is the
 *   index of the first slot whose address is not in T, or the number of whole slots that fit (P(k) + 7 <= L) if there is no
 *   such slot.  After a tick slot k with (P(k) + 7) % 2048 == 2044 comes an ACK: the ack address, a bank byte, 0xff.  The bank
 *   of opcode k is bit 0 of the bank byte of the last ACK before it, 0 before the first ACK.  The stream's mode is byte 6.
 *   Status.  Of several offences the one at the lowest byte position is reported; a stream with an offence still has a
 *   well-defined n_ops and banks (BAD_LENGTH: n_ops = 0, mode = 0).
 *     IIV_A2M_BAD_LENGTH    L <= 0, L % 2048 != 0, or L above the batch's stride; position 0, nothing else is examined
 *     IIV_A2M_BAD_HEADER    a byte 0..5 is not 0xff, or byte 6 is not 0 or 1; that byte (mode reports byte 6 as it is)
 *     IIV_A2M_BAD_ACK       an ACK before slot n_ops has a wrong address, a bank byte that is not 0x54 / 0x55, or a fourth byte
 *                           that is not 0xff; the first wrong byte
 *     IIV_A2M_BAD_ADDRESS   slot n_ops exists and its address is not the terminate address; P(n_ops)
 *     IIV_A2M_NO_TERMINATE  no slot n_ops fits; P(n_ops)
 *     IIV_A2M_BAD_PADDING   a non-zero byte behind Terminate (from P(n_ops) + 2 on): that byte; or L is not P(n_ops) + 2
 *                           rounded up to a multiple of 2048: that rounded value
 * The reader owns the device copy of the table the kernels look addresses up in (65 536 x u16); one owner, destroyed once,
 * not while a call that uses it is in flight.  Creation refuses (IIV_ERR_INVALID, before the device is touched) addresses
 * that are not pairwise distinct among the 1024 tick addresses, the ack and the terminate address. */
#define IIV_A2M_OK 0
#define IIV_A2M_BAD_LENGTH 1
#define IIV_A2M_BAD_HEADER 2
#define IIV_A2M_BAD_ACK 3
#define IIV_A2M_BAD_ADDRESS 4
#define IIV_A2M_NO_TERMINATE 5
#define IIV_A2M_BAD_PADDING 6

typedef struct iiv_a2m_reader iiv_a2m_reader;

int iiv_a2m_reader_create(const uint16_t tick_addr[1024], uint16_t ack_addr, uint16_t terminate_addr, iiv_a2m_reader **out);
void iiv_a2m_reader_destroy(iiv_a2m_reader *reader);

/* Whole slots in a stream of `length` bytes: the largest n_ops a stream of that length can have.  Host only, closed form. */
long iiv_a2m_max_ops(size_t length);

/* The three calls below take n_streams streams at d_bytes + s * stride (stride >= 2048; every byte of a row up to its length is
 * read, none behind it).  They are asynchronous on `stream` and allocate nothing.  IIV_ERR_INVALID before anything is launched,
 * with nothing written: a NULL reader or pointer (d_init_main / d_init_aux may be NULL), n_streams < 0, stride < 2048, a bad
 * alignment, a bad count.  n_streams == 0 succeeds and writes nothing.
 *
 * iiv_a2m_scan: d_lengths is int64 [n_streams], d_info int64 [n_streams][4] = {status, mode, n_ops, position}, both on the
 * device and 8-byte aligned.  Slots and ACKs are checked one thread each; the lowest position is found by a minimum over
 * values that depend on the bytes alone, so the result does not depend on scheduling. */
int iiv_a2m_scan(const iiv_a2m_reader *reader, int n_streams, const uint8_t *d_bytes, size_t stride, const int64_t *d_lengths,
                 int64_t *d_info, void *stream);

/* The inverse of iiv_emit_stream.  For every stream the first n_ops (of d_info, a scan's output, whatever its status) opcodes as
 * the encoder's 6-byte records {page, content, four offsets} at d_ops + s * ops_stride, their ticks (4..66) at
 * d_ticks + s * ticks_stride and their banks (0 / 1) at d_banks + s * ticks_stride.  Bytes past n_ops are left alone.
 * ops_stride >= 6 * iiv_a2m_max_ops(stride) and ticks_stride >= iiv_a2m_max_ops(stride), so that no d_info can take a write
 * out of a row. */
int iiv_a2m_decode(const iiv_a2m_reader *reader, int n_streams, const uint8_t *d_bytes, size_t stride, const int64_t *d_info,
                   uint8_t *d_ops, size_t ops_stride, uint8_t *d_ticks, uint8_t *d_banks, size_t ticks_stride, void *stream);

/* Snapshot j, j < n_snaps, is the 2 x 8 KiB of screen memory after the first min(first_snap + j * snap_every, n_ops) opcodes of
 * the stream: opcodes apply in stream order, each storing its content byte at its four offsets of its page, in its bank --
 * replay follows the bank bytes and does not read the mode, so d_aux is always written (all initial state for a well-formed
 * HGR stream).  The starting state is d_init_main / d_init_aux [n_streams][32][256], NULL = zeros.  d_main / d_aux are
 * [n_streams][n_snaps][32][256]; they and the initial maps are 8-byte aligned, so a snapshot tensor goes straight into
 * iiv_render_rgb and iiv_render_error.  first_snap >= 0, snap_every >= 1, n_snaps >= 1.  An opcode takes 73 cycles whatever it
 * does, so uniform sampling in opcodes is uniform sampling in time. */
int iiv_a2m_replay(const iiv_a2m_reader *reader, int n_streams, const uint8_t *d_bytes, size_t stride, const int64_t *d_info,
                   long first_snap, long snap_every, int n_snaps, const uint8_t *d_init_main, const uint8_t *d_init_aux,
                   uint8_t *d_main, uint8_t *d_aux, void *stream);

/* ==== f10: direct ingest ====================================================
 * RGB frames -> memory maps chosen THROUGH the colour model: the reference README's "direct image encoding".  f3 picks, per
 * 140-wide colour pixel, the nearest colour and writes its aligned dot quad; the screen shows a sliding four-dot window (f7),
 * so every boundary between two different quads shows dots of colours nobody chose.  Here every screen row gets the byte row
 * whose RENDERED dots are nearest the source.  Rows are independent, the arithmetic is integer, and the rule is global, so
 * every implementation agrees byte for byte (tests/direct_model.py restates it in numpy and is held to it by exhaustive
 * search through tests/render_model.py; csrc/iiv_direct.hip computes it).
 *   Source.  d_rgb is [n][192][ref_width][3] u8, ref_width 280 or 560; as in f8, R[y][x][c] = rgb[y][x * ref_width / 560][c] for
 *   dot x in 0..559.
 *   Target.  T[y][x][c] = clamp(R[y][x][c] + floor((2 * B[y & 3][(x >> 2) & 3] - 15) * dither / 16), 0, 255), B the 4x4 Bayer
 *   matrix of f3, dither 0..255 (indexed by the quad x >> 2: f3's colour pixel k).  IIV_DITHER_DIFFUSION is refused.
 *   What a byte row shows is exactly f7: the row's bytes (DHGR: 80, aux[0], main[0], aux[1], ...; HGR: 40) give the dots by
 *   f7's rules -- HGR's palette-bit shift, bit 6 of the byte to the left and the dropped 561st dot included -- and dot x shows
 *   value(x) = rol4(w, (x + 1) & 3), w as in f7, dots left of the row 0.
 *   Cost of a byte row: the sum over x < 560, c < 3 of (palette_rgb[3 * value(x) + c] - T[y][x][c])^2 (at most 560 * 3 * 255^2).
 *   The row written: among all byte rows with bit 7 clear (DHGR), or all byte rows (HGR: bit 7 is the palette bit), one of
 *   least cost; among several of least cost the one whose value sum b[i] * 256^i is smallest, i the byte's position in the
 *   sequence above (the last byte is the most significant).
 *   Bytes land at y_to_base_addr (screen.py:16-22); the screen holes are written as 0; d_aux is ignored in HGR.
 *   d_cost, if not NULL, is [n] uint64 and is overwritten with the sum of the frame's 192 row costs.  With dither 0 that is
 *   iiv_render_error's level 0 of the maps written, summed over the channels -- and no memory map has a smaller one.
 * d_rgb 4-byte aligned, d_main / d_aux / d_cost 8-byte aligned.  Asynchronous on `stream`; the palette is read before the call
 * returns; nothing is allocated.  n_frames == 0 succeeds and writes nothing.  IIV_ERR_INVALID before anything is launched,
 * with nothing written: a bad mode, n_frames < 0, a NULL palette_rgb, d_rgb or d_main, a NULL d_aux in DHGR, ref_width not
 * 280 or 560, dither outside 0..255, a bad alignment. */
int iiv_frames_to_memory_maps_direct(int mode, const uint8_t palette_rgb[48], int n_frames, const uint8_t *d_rgb, int ref_width,
                                     int dither, uint8_t *d_main, uint8_t *d_aux, uint64_t *d_cost, void *stream);

/* ==== f11: YUV 4:2:0 sources ================================================
 * Decoders deliver 4:2:0 YCbCr (ffmpeg's yuv420p = I420, hardware decoders' NV12), not the packed RGB f5 takes.  This entry
 * point is f5 on the RGB frame that the planes DEFINE, integer arithmetic only, so every implementation agrees byte for byte
 * (tests/yuv_model.py restates it in numpy; csrc/iiv_resize.hip computes it).  For source pixel (x, y) of an
 * h x w frame, >> arithmetic:
 *     Yv = Y[y][x]                      Y plane: h rows of w bytes
 *     U  = Cb[y >> 1][x >> 1]           chroma planes: (h + 1) / 2 rows of (w + 1) / 2 samples
 *     V  = Cr[y >> 1][x >> 1]           (the NEAREST sample: no chroma interpolation, no siting -- stated, not an accident)
 *     c  = Yv - y_off,  d = U - 128,  e = V - 128
 *     R  = clamp((ky c        + rv e + 128) >> 8, 0, 255)
 *     G  = clamp((ky c + gu d + gv e + 128) >> 8, 0, 255)
 *     B  = clamp((ky c + bu d        + 128) >> 8, 0, 255)
 * and that RGB frame goes through f5 exactly as iiv_resize_frames takes it: the same coefficients, passes, pass order and
 * rounding.  matrix = (y_off, ky, rv, gu, gv, bu): y_off 0..255 and every coefficient in -1023..1023, else IIV_ERR_INVALID;
 * every sum is then at most 3 * 1023 * 255 + 128 < 2^20 in magnitude -- int32 with eleven bits to spare.  BT.601 limited range
 * is (16, 298, 409, -100, -208, 516), BT.709 limited (16, 298, 459, -55, -136, 541), full-range JFIF (0, 256, 359, -88, -183,
 * 454) (frame_grabber.YUV_MATRICES).
 * Planes (all strides in bytes, no alignment required; rows and frames of a plane must not overlap):
 *     Y  of frame f, row y, pixel x   at d_y + f * y_frame_stride + y * y_row_stride + x
 *     Cb of frame f, row j, sample i  at d_u + f * c_frame_stride + j * c_row_stride + i * c_pixel_stride, Cr the same from d_v
 * c_pixel_stride is 1 for planar I420 / YV12 and 2 for the interleaved plane of NV12 (d_v = d_u + 1) / NV21 (d_u = d_v + 1);
 * any other value is IIV_ERR_INVALID.  No byte outside the planes' rows influences the result.
 * -> d_dst [n][H][W][3] contiguous.  Limits, errors (before anything is launched) and the stream contract are
 * iiv_resize_frames' own, and so are the coefficient tables: one cache per (device, in, out) serves both entry points, the FIRST
 * call with a size pair on a device builds and uploads them synchronously, every later call is asynchronous on `stream` with
 * stream-ordered scratch.  `matrix` is read before the call returns.  Where the horizontal pass comes first (W != w, and not
 * both H != h and h > 100 w -- every video shape) the conversion happens inside that pass and the full-size RGB frame never
 * exists in memory; otherwise a conversion kernel writes a bounded chunk of RGB frames to scratch in front of the RGB path. */
int iiv_resize_frames_yuv420(int n, int h, int w, const uint8_t *d_y, size_t y_frame_stride, size_t y_row_stride,
                             const uint8_t *d_u, const uint8_t *d_v, size_t c_frame_stride, size_t c_row_stride, int c_pixel_stride,
                             const int32_t matrix[6], int H, int W, uint8_t *d_dst, void *stream);

/* ==== f12: fitting a frame to the screen: boxed resize, letterbox and crop ======
 * f5 stretches every source over the whole destination.  These entry points resize a BOX of the source into a RECTANGLE of the
 * destination and give the rest of the destination a fill colour, byte for byte as Pillow's
 * Image.resize((rw, rh), LANCZOS, box=(x0, y0, x1, y1)) pasted at (rx, ry) onto a canvas of the fill colour (DESIGN.md 28;
 * tests/fit_model.py restates it; observed on Pillow 12.2.0).  What the box changes in f5, per axis (in = the frame's size on
 * that axis, in0 / in1 = the box's ends, out = rw or rh):
 *   1. the box is four float32 values: anything wider is rounded to float32 first;
 *   2. scale = (double)(in1 - in0) / out, the subtraction IN FLOAT32 and only then widened;
 *   3. center = in0 + (xx + 0.5) scale in float64 (in0 the float32 value widened); filterscale, support, ksize, the weights,
 *      their normalisation and the 22-bit rounding as in f5 with that scale; xmin is clamped at 0 and xmin + count at `in`,
 *      the FRAME's size, not at the box: taps reach past the box into the picture around it;
 *   4. an axis gets a pass when out != in or in0 != 0 or in1 != in; the horizontal pass comes first, the vertical one when the
 *      frame (not the box) has h > 100 w; an integer-aligned box of the rectangle's own size yields identity coefficients (Pillow
 *      crops; the pass gives the same bytes).
 * box = (x0, y0, x1, y1) with 0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h as float32 (an empty box, which Pillow accepts, is
 * refused); rect = (rx, ry, rw, rh) inside the H x W destination with rw, rh >= 1; fill = r | g << 8 | b << 16 (< 2^24); any
 * other value is IIV_ERR_INVALID before anything is launched.  box = (0, 0, w, h) with rect = (0, 0, W, H) is f5 itself, byte
 * for byte.  Only the source columns and rows that the two tables touch are read.  Limits, the stream contract and the
 * stream-ordered scratch are iiv_resize_frames' own; the coefficient cache is keyed by (device, in, bits of in0, bits of in1, out)
 * and serves all four entry points: the FIRST call with a geometry on a device is synchronous, every later one asynchronous. */

/* iiv_resize_coeffs for the box [in_box[0], in_box[1]) of an axis of in_size samples (rules 1 to 3), host only (no device).
 * 0 <= in_box[0] < in_box[1] <= in_size, else IIV_ERR_INVALID.  in_box = (0, in_size) gives iiv_resize_coeffs' table. */
int iiv_resize_coeffs_box(int in_size, const float in_box[2], int out_size, int *ksize, int32_t *bounds, int32_t *coeffs);

/* iiv_resize_frames of the box into the rectangle: d_dst [n][H][W][3] contiguous holds, inside rect, the boxed resize of source
 * frame f and the fill colour everywhere else (nothing extra is launched when rect is the whole destination). */
int iiv_resize_frames_fit(int n, int h, int w, const uint8_t *d_src, size_t frame_stride, size_t row_stride, const float box[4],
                          int H, int W, const int rect[4], uint32_t fill, uint8_t *d_dst, void *stream);

/* The same for 4:2:0 planes (f11): the planes define an RGB frame over the WHOLE h x w source, chroma taken at (y >> 1, x >> 1)
 * of absolute source coordinates, and the box is applied to that frame -- an odd x0 or y0 is well defined. */
int iiv_resize_frames_yuv420_fit(int n, int h, int w, const uint8_t *d_y, size_t y_frame_stride, size_t y_row_stride,
                                 const uint8_t *d_u, const uint8_t *d_v, size_t c_frame_stride, size_t c_row_stride,
                                 int c_pixel_stride, const int32_t matrix[6], const float box[4], int H, int W, const int rect[4],
                                 uint32_t fill, uint8_t *d_dst, void *stream);

/* ==== f13: speaker preview ==================================================
 * What a stream's ticks sound like: the 1-bit signal the player's speaker toggles make, taken down to 16-bit PCM by a CIC
 * decimator -- f7 for the ear.  Integer arithmetic only, so every implementation agrees sample for sample
 * (tests/speaker_model.py restates this section cycle by cycle; csrc/iiv_speaker.hip computes it).
 *   Periods.  Time is cut into periods of 73 cycles (the player's opcode, player/main.s).  Tick opcode k is one period: the
 *   speaker is toggled at its start and width(tick) cycles later, so the level is high for width cycles and low for the rest.
 *   width(t) = t for the even t in 4..66, except width(22) = 21 and width(40) = 41 (the two opcodes whose pulse is a cycle
 *   off).  A tick byte that is not an even number in 4..66 has width 0 and sets *d_err = 1 (d_err: device int, may be NULL, as
 *   for iiv_emit_chunk; the call never clears it).
 *   ACKs.  By f9's layout an ACK follows opcodes 290, 582, 874, ...; it is two more periods of width 34 each.  The ACKs in
 *   front of opcode k: A(k) = 0 for k < 291, 1 + (k - 291) / 292 otherwise.  Opcode k is period q(k) = k + 2 A(k); a stream of n
 *   opcodes has Q(n) = n + 2 A(n) periods.  W[p] is the width of period p.
 *   Left out on purpose: the header, NOP and Terminate opcodes, the player's wait loop when the network is late, and the
 *   key-press pause are not part of the signal.
 *   Signal.  x(c) = +1 if 0 <= c < 73 Q and c % 73 < W[c / 73], else -1, for every integer c: before and after the stream the
 *   speaker rests low.
 *   Filter.  h_1 is `decim` ones, h_r = h_(r-1) * h_1 (convolution): r (decim - 1) + 1 taps that sum to decim^r.
 *     acc[m] = sum over i of h_order[i] * x(m * decim + decim - 1 - i)     for 0 <= m < M = ceil(73 Q / decim), M = 0 when n = 0
 *   Scaling.  pcm[m] = clamp(floor(acc[m] * gain / decim^order), -32768, 32767), the floor towards minus infinity, the product
 *   in 64 bits (73^4 * 32767 does not fit 32).
 *   Limits.  1 <= decim <= 73, 1 <= order <= 4, 0 <= gain <= 32767.
 * The output rate is the machine's clock over decim; the clock itself is the caller's business (audio.speaker_rate). */

/* Q(n_ops) and M(n_ops, decim): host only, closed forms.  n_ops < 0 counts as 0; a decim outside 1..73 is IIV_ERR_INVALID. */
long iiv_speaker_periods(long n_ops);
long iiv_speaker_sample_count(long n_ops, int decim);

/* The PCM of n_streams streams: stream s has the tick bytes d_ticks + s * ticks_stride (what iiv_a2m_decode and iiv_audio_ticks
 * write), its opcode count at d_counts[s * counts_stride] -- a device int64, 8-byte aligned, so a scan's d_info + 2 with stride 4
 * goes in as it is; a negative count is read as 0, one above ticks_stride as ticks_stride -- and gets its M(s) samples at
 * d_pcm + s * pcm_stride (in samples; 2-byte aligned; rows that start 16-byte aligned are written 16 bytes a lane).  Samples past
 * M(s) are left alone.  pcm_stride >= iiv_speaker_sample_count(ticks_stride, decim), so that no count can take a write out of a
 * row.  Asynchronous on `stream`; nothing is allocated, nothing synchronised, no host memory is read after the call returns (the
 * filter's running sum, at most 290 ints, goes to the kernel by value).  n_streams == 0 succeeds and writes nothing.
 * IIV_ERR_INVALID before anything is launched, with nothing written: a limit above, n_streams < 0, a NULL d_ticks, d_counts or
 * d_pcm, a bad alignment, a ticks_stride above 2^48, a pcm_stride that is too small. */
int iiv_speaker_pcm(int n_streams, const uint8_t *d_ticks, size_t ticks_stride, const int64_t *d_counts, size_t counts_stride,
                    int decim, int order, int gain, int16_t *d_pcm, size_t pcm_stride, int *d_err, void *stream);

/* ==== f14: temporal hold ====================================================
 * The first front-end step along the time axis: a pixel that a viewer calls still keeps its bytes from frame to frame, so that
 * sensor noise, compression ripple and a resampler's jitter are not priced and queued as differences.  It sits in front of every
 * converter (f3, f6, f10) and changes none of them: where the frame carries the value of the frame before, the ordered dither,
 * the mono dither and `direct` write the same bytes, and the error diffusions do wherever everything above and to the left is
 * unchanged as well.  Integer arithmetic only, so every implementation agrees byte for byte (tests/temporal_model.py restates
 * this section in numpy; csrc/iiv_temporal.hip computes it).
 *   A clip is n_frames frames of `pixels` RGB pixels, 3 bytes each, dense within a frame.  Per clip there is one held frame h
 *   (pixels * 3 bytes).  Per pixel, for frames t = 0, 1, ... in order, x the source pixel and y the output pixel:
 *     if `first` is set and t == 0:  y = x, h = x; the pixel counts as passed.
 *     otherwise  d = max(|x.r - h.r|, |x.g - h.g|, |x.b - h.b|)
 *                w(d) = 0                                    for d <= lo     (y == h: held)
 *                w(d) = 256                                  for d > hi      (y == x: passed)
 *                w(d) = floor(256 (d - lo) / (hi - lo + 1))  between         (1..255: blended)
 *                y_c = h_c + (((x_c - h_c) * w + 128) >> 8)  per channel, the shift arithmetic: floor towards minus infinity
 *                h = y
 *   d is taken against the HELD value, not against the previous source frame: a slow fade gets through once it has moved more
 *   than lo -- hysteresis, not a freeze.  lo = hi = 0 is the identity, byte for byte.
 *   Counts.  Per (clip, frame) three uint32: pixels held (d <= lo), blended (lo < d <= hi), passed (d > hi, and every pixel of a
 *   `first` frame 0).  They sum to `pixels`.
 * Frame t of clip k is read at d_src + k * src_clip_stride + t * src_frame_stride and written at d_out + k * out_clip_stride +
 * t * out_frame_stride (strides in bytes).  d_state is [n_clips] held frames, clip k's at d_state + k * state_stride: with `first`
 * they are only written, without it they are read and then written -- the h behind the call's last frame --, which is how a clip
 * continues across calls.  d_counts is [n_clips][n_frames][3], dense, and may be NULL; every entry is written by the call, the
 * caller clears nothing.  d_out == d_src with equal strides is allowed; any other overlap is the caller's error, and d_state
 * overlaps nothing.
 * IIV_ERR_INVALID before anything is launched, with nothing written: n_clips or n_frames < 0; pixels not a positive multiple of 4
 * (or above 2^40); a pointer or a stride that is not 4-byte aligned; a frame stride below pixels * 3; with more than one clip a
 * state_stride below pixels * 3; lo or hi outside 0..255, or lo > hi; a NULL d_src, d_out or d_state where there is work.
 * n_clips == 0 or n_frames == 0 succeeds and touches nothing.  Asynchronous on `stream`; nothing is allocated, nothing
 * synchronised, nothing kept between calls, no host memory is read after the call returns (w(d), 256 entries, goes to the kernel
 * by value); the clearing of d_counts is issued on `stream` in front of the kernel. */
int iiv_temporal_hold(int n_clips, int n_frames, long pixels, const uint8_t *d_src, size_t src_clip_stride, size_t src_frame_stride,
                      uint8_t *d_out, size_t out_clip_stride, size_t out_frame_stride, uint8_t *d_state, size_t state_stride,
                      int first, int lo, int hi, uint32_t *d_counts, void *stream);

/* ==== f15: picture levels ===================================================
 * What the audio track has had since f4 (a factor from the 0.5th and 99.5th percentiles of the PCM) for the picture: a histogram
 * per frame, black and white points from it, and a per-channel table with a 3 x 3 matrix behind it -- levels, gamma, brightness,
 * contrast and saturation in one pass.  The stage sits behind the resize (f5, f11, f12) and in front of the temporal hold (f14),
 * so the hold's thresholds are in the values the converters see; it changes no converter.  Integer arithmetic only, so every
 * implementation agrees byte for byte (tests/levels_model.py restates this section in numpy; csrc/iiv_levels.hip computes it;
 * DESIGN.md 31).  The curves themselves (gamma, contrast) are the caller's: the ABI takes tables, so no pow() has to agree across
 * libraries (frame_grabber.levels_lut, frame_grabber.saturation_matrix).
 *   A clip is laid out as in f14: n_frames frames of `pixels` RGB pixels, 3 bytes each, dense within a frame; frame t of clip k
 *   is at d + k * clip_stride + t * frame_stride (strides in bytes).
 *   Luma.  Y = (77 R + 150 G + 29 B + 128) >> 8; the weights sum to 256, so Y is 0..255. */

/* The histograms of every frame: d_hist is [n_clips][n_frames][4][256] uint32, dense, channel order R, G, B, Y; entry v of a
 * channel is the number of the frame's pixels whose channel has the value v, so each channel sums to `pixels`.  Per frame, so
 * that the caller chooses which frames to sum.  Every entry is written by the call; the caller clears nothing.
 * IIV_ERR_INVALID before anything is launched, with nothing written: n_clips or n_frames < 0; pixels not a positive multiple of 4,
 * or above 2^31 (a count fits its uint32); a pointer or a stride that is not 4-byte aligned; a frame stride below pixels * 3; a
 * NULL d_src or d_hist where there is work.  n_clips == 0 or n_frames == 0 succeeds and touches nothing.  Asynchronous on
 * `stream`; nothing is allocated, nothing synchronised, nothing kept between calls, no host memory is read after the call
 * returns; nothing but the one kernel is issued (no clearing, no global atomics: a frame is one workgroup's). */
int iiv_levels_histogram(int n_clips, int n_frames, long pixels, const uint8_t *d_src, size_t src_clip_stride,
                         size_t src_frame_stride, uint32_t *d_hist, void *stream);

/* Black and white points from one histogram of 256 counts (one channel of the above, summed over the frames the caller chose):
 * host only, a closed form.  total = sum of hist, cum(v) = sum of hist[u] for u <= v, cum(-1) = 0;
 * k_lo = floor(total * lo_ppm / 10^6), k_hi = floor(total * hi_ppm / 10^6);
 *   *black = the least v with cum(v) > k_lo             (at most k_lo pixels lie below it)
 *   *white = the greatest v with total - cum(v - 1) > k_hi   (at most k_hi pixels lie above it)
 * total == 0 or white <= black gives (0, 255), the identity range.  IIV_ERR_INVALID: lo_ppm or hi_ppm above 500000, a total
 * above 2^43 (the products stay inside uint64), a NULL pointer. */
int iiv_levels_auto(const uint64_t hist[256], uint32_t lo_ppm, uint32_t hi_ppm, int *black, int *white);

/* The tables applied.  Clip k has a table lut[3][256] uint8 at d_lut + k * lut_stride and a matrix m[3][3] int16 (rows of 3,
 * dense: 18 bytes) at (const uint8_t *)d_matrix + k * matrix_stride; a stride of 0 means one table or matrix for all clips, any
 * other lut_stride is at least 768 and any other matrix_stride at least 20, and both are multiples of 4.  Per pixel x -> y:
 *     a_c = lut[c][x_c]
 *     y_c = clamp((m[c][0] a_0 + m[c][1] a_1 + m[c][2] a_2 + 128) >> 8, 0, 255)      the shift arithmetic
 * The matrix is Q8: entries lie in -2048..2047 (+-8.0).  The call cannot check that without reading device memory: the Python
 * layer checks it before upload, and for an entry outside that range the kernel computes the formula in int32 all the same
 * (3 * 32768 * 255 + 128 < 2^31).  The identity table with 256 * I is the identity, byte for byte.  d_out == d_src with equal
 * strides is allowed; any other overlap is the caller's error.
 * IIV_ERR_INVALID before anything is launched, with nothing written: as for iiv_levels_histogram (pixels up to 2^40 as in f14; the
 * frame strides of d_src and d_out both), and the stride rules above; a NULL d_src, d_out, d_lut or d_matrix where there is work.
 * n_clips == 0 or n_frames == 0 succeeds and touches nothing.  Asynchronous on `stream`; nothing is allocated, nothing
 * synchronised, nothing kept between calls, no host memory is read after the call returns. */
int iiv_levels_apply(int n_clips, int n_frames, long pixels, const uint8_t *d_src, size_t src_clip_stride, size_t src_frame_stride,
                     uint8_t *d_out, size_t out_clip_stride, size_t out_frame_stride, const uint8_t *d_lut, size_t lut_stride,
                     const int16_t *d_matrix, size_t matrix_stride, void *stream);

/* ==== f16: spatial filter ===================================================
 * The first front-end step that looks at a pixel's neighbours: a separable 5 x 5 blur B of the frame, and per pixel a gain on the
 * difference between the pixel and B, chosen by the size of that difference.  A negative gain where the difference is small pulls
 * noise to the neighbourhood's mean and leaves an edge alone (denoise); a positive gain where it is large is an unsharp mask.  The
 * stage sits behind the levels (f15) and in front of the temporal hold (f14), so both thresholds are in the values the converters
 * see and the hold sees the denoised picture; it changes no converter.  Integer arithmetic only, so every implementation agrees
 * byte for byte (tests/spatial_model.py restates this section in numpy; csrc/iiv_filter.hip computes it).
 *   A clip is laid out as in f14 and f15, but the frame's geometry matters: a frame is `height` rows of `width` RGB pixels, 3 bytes
 *   each, rows dense (width * 3 bytes); frame t of clip k is at d + k * clip_stride + t * frame_stride (strides in bytes).
 *   Coordinates outside the frame are clamped to it: the edge is replicated.
 *   taps_x[5] and taps_y[5] are 0..256 each and sum to exactly 256 per axis; gain[256] is Q8, each entry in -256..1024.  Per frame,
 *   per channel c, p the source:
 *     h_c(x, y) = sum_{k=0..4} taps_x[k] * p_c(clamp(x + k - 2, 0, width - 1), y)                        (0..65280: fits a uint16)
 *     B_c(x, y) = (sum_{j=0..4} taps_y[j] * h_c(x, clamp(y + j - 2, 0, height - 1)) + 32768) >> 16       (0..255)
 *     d_c = p_c - B_c
 *     m   = max(|d_r|, |d_g|, |d_b|)                            one index per pixel, as f14 takes one d per pixel
 *     y_c = clamp(p_c + ((gain[m] * d_c + 128) >> 8), 0, 255)   the shift arithmetic: floor towards minus infinity
 *   gain == 0 everywhere is the identity, and so are the taps (0, 0, 256, 0, 0) on both axes whatever the gain; gain == -256
 *   everywhere gives y == B, the plain blur; a constant frame is a fixed point.
 * IIV_ERR_INVALID before anything is launched, with nothing written, in this order: n_clips or n_frames < 0; height * width not a
 * positive multiple of 4, or above 2^24; d_src, d_out or a stride that is not 4-byte aligned; a frame stride below height * width *
 * 3; then height outside 1..4096; width outside 4..4096 or not a multiple of 4; NULL taps_x, taps_y or gain; a tap above 256, or
 * an axis whose taps do not sum to 256; a gain outside -256..1024; d_out == d_src (a neighbour's source would be overwritten: in
 * place is not possible here; any other overlap is the caller's error); a NULL d_src or d_out where there is work.
 * n_clips == 0 or n_frames == 0 succeeds and touches nothing.  Asynchronous on `stream`; nothing is allocated, nothing
 * synchronised, nothing kept between calls, no host memory is read after the call returns (the taps and the gain go to the kernel
 * by value); nothing but the one kernel is issued. */
int iiv_filter_frames(int n_clips, int n_frames, int height, int width, const uint8_t *d_src, size_t src_clip_stride,
                      size_t src_frame_stride, uint8_t *d_out, size_t out_clip_stride, size_t out_frame_stride,
                      const uint16_t taps_x[5], const uint16_t taps_y[5], const int16_t gain[256], void *stream);

#ifdef __cplusplus
}
#endif
#endif
