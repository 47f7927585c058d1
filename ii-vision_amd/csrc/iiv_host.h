// iiv_host.h -- what the translation units of libiivision.so share on the host side (the C ABI itself is include/iivision.h):
// the error idioms, the checked kernel launch, the owners of device memory, pinned memory and events, and the prototypes of
// the functions one file calls in another.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <utility>

#include "../../include/iivision.h"
#include "iiv_device.h"

namespace iiv {

int set_error(int code, const char *fmt, ...);
int hip_check(hipError_t e, const char *what);

#define IIV_HIP(expr)                                    \
    do {                                                 \
        int _rc = ::iiv::hip_check((expr), #expr);       \
        if (_rc) return _rc;                             \
    } while (0)

// ---- how a kernel is launched: launch() enqueues it and returns hip_check of the launch under `label` ("table_kernel launch":
// the label names the kernel, iiv_last_error() quotes it), so every launch is checked on its own --
//     if (int rc = launch(by_mode(mode, k<kDHGR>, k<kHGR>), "k launch", grid, dim3(256), 0, st, args...)) return rc;
// P... comes from the kernel alone and the arguments convert to it as in a direct call: a literal, a size_t or a struct
// by reference at the call site reaches the kernel as the type the kernel declares.
template <typename T> struct KernelParam { using type = T; };
template <typename... P>
int launch(void (*kernel)(P...), const char *label, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st,
           typename KernelParam<P>::type... args)
{
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, st, args...);
    return hip_check(hipGetLastError(), label);
}

// a kernel template's instance for `mode` (k<kDHGR> and k<kHGR> have one function type).  DHGR is named first: the device
// code of a file's instances is emitted in the order the host code first names them.
template <typename K> K by_mode(int mode, K dhgr, K hgr) { return mode == kDHGR ? dhgr : hgr; }

// ---- owners of the synchronous HIP resources (host-only).  Each is move-only (a declared move makes the copies deleted),
// empty when default-constructed, and releases what it holds in its destructor, ignoring the status.  Stream-ordered memory
// (hipMallocAsync / hipFreeAsync) follows another rule -- freed behind the work on its stream, scoped to the call -- and is
// not held in these.

// `count` elements of T from hipMalloc
template <typename T> class DeviceBuf {
public:
    DeviceBuf() = default;
    DeviceBuf(DeviceBuf &&o) noexcept { swap(o); }
    DeviceBuf &operator=(DeviceBuf &&o) noexcept { swap(o); return *this; }   // (what this one held goes with `o`)
    ~DeviceBuf() { reset(); }
    int alloc(size_t count, const char *what)   // frees what it held first; stays empty if the allocation fails
    {
        reset();
        const int rc = hip_check(hipMalloc(&p_, count * sizeof(T)), what);
        if (rc) p_ = nullptr;
        else n_ = count;
        return rc;
    }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr, n_ = 0; }
    T *release() { T *p = p_; p_ = nullptr, n_ = 0; return p; }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t count() const { return n_; }

private:
    void swap(DeviceBuf &o) { std::swap(p_, o.p_), std::swap(n_, o.n_); }
    T *p_ = nullptr;
    size_t n_ = 0;
};

// one counter on the device for the kernels that count mismatches: zero() on `st` before they are launched, read() after
class DeviceCounter {
public:
    int zero(hipStream_t st)
    {
        if (int rc = d_.alloc(1, "hipMalloc(count)")) return rc;
        IIV_HIP(hipMemsetAsync(d_, 0, sizeof(unsigned long long), st));
        return IIV_OK;
    }
    int read(unsigned long long *out, hipStream_t st)   // synchronises `st`
    {
        IIV_HIP(hipMemcpyAsync(out, d_, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        IIV_HIP(hipStreamSynchronize(st));
        return IIV_OK;
    }
    operator unsigned long long *() const { return d_; }

private:
    DeviceBuf<unsigned long long> d_;
};

// the same from hipHostMalloc(flags): pinned / coherent host memory
template <typename T> class HostBuf {
public:
    HostBuf() = default;
    HostBuf(HostBuf &&o) noexcept { swap(o); }
    HostBuf &operator=(HostBuf &&o) noexcept { swap(o); return *this; }
    ~HostBuf() { reset(); }
    int alloc(size_t count, unsigned flags, const char *what)
    {
        reset();
        const int rc = hip_check(hipHostMalloc(&p_, count * sizeof(T), flags), what);
        if (rc) p_ = nullptr;
        else n_ = count;
        return rc;
    }
    void reset() { if (p_) (void)hipHostFree(p_); p_ = nullptr, n_ = 0; }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t count() const { return n_; }

private:
    void swap(HostBuf &o) { std::swap(p_, o.p_), std::swap(n_, o.n_); }
    T *p_ = nullptr;
    size_t n_ = 0;
};

// an event from hipEventCreateWithFlags
class Event {
public:
    Event() = default;
    Event(Event &&o) noexcept { std::swap(ev_, o.ev_); }
    Event &operator=(Event &&o) noexcept { std::swap(ev_, o.ev_); return *this; }
    ~Event() { reset(); }
    int create(unsigned flags, const char *what)
    {
        reset();
        const int rc = hip_check(hipEventCreateWithFlags(&ev_, flags), what);
        if (rc) ev_ = nullptr;
        return rc;
    }
    void reset() { if (ev_) (void)hipEventDestroy(ev_); ev_ = nullptr; }
    operator hipEvent_t() const { return ev_; }

private:
    hipEvent_t ev_ = nullptr;
};

// iiv_tables.hip
int cie2000_matrix(const uint8_t rgb[48], double out_f[256], int32_t out_i[256], hipStream_t st);
int symmetrise_table(int mode, uint16_t *d_table, hipStream_t st);
int store_table_from_table(int mode, const uint16_t *d_table, uint16_t *d_store, hipStream_t st);
int delta_e_pairs(int n, const double *lab1, const double *lab2, double *out, hipStream_t st);
int pixel_strings(int mode, uint32_t *d_dots, uint8_t *d_pixels, ulonglong2 *d_strings, hipStream_t st);
int build_table(int mode, const int32_t dm[256], uint16_t *d_out, int symmetric, hipStream_t st);
int build_store_table(int mode, const int32_t dm[256], uint16_t *d_out, hipStream_t st);
int build_strings(int mode, const int32_t dm[256], DeviceBuf<ulonglong2> &d_strings, DeviceBuf<uint16_t> &d_sub, hipStream_t st);
int build_hgr_dot_lut(DeviceBuf<uint32_t> &d_out, hipStream_t st);   // HGR: windows -> dots, two lookups (iiv_edit.h: hgr_dot_slot_lo)
int check_dw_piece_table(int mode, const int32_t dm[256], const uint16_t *d_table, unsigned long long *mismatches, hipStream_t st);
int build_dw_piece_table(int mode, const uint16_t *d_sub, DeviceBuf<uint32_t> &d_out, hipStream_t st);   // DHGR: [2 banks][4096] u32; HGR: [4096]
size_t split_entries(int mode, int right);
int build_split_tables(int mode, const ulonglong2 *d_strings, const uint16_t *d_sub, uint32_t *d_left, uint32_t *d_right,
                       hipStream_t st);
struct NarrowTables;
int build_narrow_tables(int mode, const ulonglong2 *d_strings, const uint16_t *d_sub, const uint32_t *d_left, const uint16_t *d_store,
                        NarrowTables *out, DeviceBuf<uint8_t> &storage, hipStream_t st);   // (out->base points into `storage`)
int expand_narrow_tables(int mode, const NarrowTables &nt, const uint16_t *d_store, uint16_t *d_out, unsigned long long *n_mismatch,
                         hipStream_t st);
int build_narrow_store_table(int mode, const int32_t dm[256], const uint16_t *d_store, uint16_t *d_expanded,
                             unsigned long long *n_mismatch, hipStream_t st);
int transpose_split_tables(int mode, const uint32_t *d_left, const uint32_t *d_right, uint32_t *d_left_t,
                           uint32_t *d_right_t, hipStream_t st);
int build_joint_tables(int mode, const NarrowTables &nt, DeviceBuf<uint32_t> &d_jl, DeviceBuf<uint32_t> &d_jr, hipStream_t st);
size_t split_dw_entries(int mode, int right);
int build_split_dw_tables(int mode, const ulonglong2 *d_strings, const uint16_t *d_sub, uint32_t *d_left, uint32_t *d_right,
                          hipStream_t st);
int check_split_dw_table(int mode, const int32_t dm[256], const uint16_t *d_table, unsigned long long *mismatches,
                         hipStream_t st);
int build_split_store_table(int mode, const int32_t dm[256], uint32_t *d_left, uint32_t *d_right, uint16_t *d_expanded,
                            hipStream_t st);

// iiv_bitmap.hip
int pack(int mode, int n, const uint8_t *d_main, const uint8_t *d_aux, uint64_t *d_packed, hipStream_t st);
int diff_weights(int mode, const uint16_t *d_table, int n, const uint64_t *d_src, const uint64_t *d_tgt,
                 int is_aux, int32_t *d_out, hipStream_t st);
int compute_delta_pages(int mode, const uint16_t *d_table, int n, const uint64_t *d_tgt, const int32_t *d_pages,
                        const int32_t *d_contents, const int32_t *d_dw_rows, int is_aux, int32_t *d_out,
                        hipStream_t st);

// iiv_render.hip: frame f's memory maps at d_main / d_aux + f * in_stride bytes
int render_rgb(int mode, const uint8_t palette_rgb[48], int n, const uint8_t *d_main, const uint8_t *d_aux, size_t in_stride,
               uint8_t *d_rgb, hipStream_t st);

// iiv_render_error.hip: the same frames against d_ref [n][192][ref_width][3] -> d_out [n][3][3]
int render_error(int mode, const uint8_t palette_rgb[48], int n, const uint8_t *d_main, const uint8_t *d_aux, size_t in_stride,
                 const uint8_t *d_ref, int ref_width, uint64_t *d_out, hipStream_t st);

}  // namespace iiv
