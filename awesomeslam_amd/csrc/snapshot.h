// snapshot.h -- include/aslam_snapshot.h: the record format on the host, and the kernels that move records between a blob and a context's
// padded layout.
//
//   record_pack<Src>  writes records: X, Z and P from a source (SnapshotSrc here: a strided gather, rows of P with stride NP -> rows with stride
//                     ld = n + 1), then the lists, the headers and the table through snap_write_lists_and_headers -- the one writer of the format
//   snapshot_unpack   the reverse scatter, which also makes the slot a FRESH one: a filter only grows in a normal run, so no filter kernel
//                     has ever seen a slot whose dimension shrank, and they rely on never-written padding staying zero.  The whole padded
//                     P, X and Z are written (zero from n on), the lists are zero beyond their counts, and the slot's share of the
//                     scratch that aslam_reset zeroes is cleared (SnapCtx::clear).
//   snapshot_gather   the record headers of a device blob, packed for one copy to the host
//
// Both movers run on a 2-D grid (row chunks, records), 16 bytes per lane and access on both sides (NP is a multiple of 16, ld is even, every
// record starts on a 64-byte boundary), at most ~2048 workgroups, grid-stride beyond.  Records of mixed n share a launch.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "device_common.h"

namespace aslam
{
constexpr int SNAP_WG = 256;
constexpr int SNAP_GRID_CAP = 2048; // workgroups per launch: 256 CUs x 8
constexpr int SNAP_CLEAR_MAX = 5;
constexpr uint32_t SNAP_VERSION = 1;
constexpr uint32_t SNAP_KNOWN_STATUS = 31; // ASLAM_ST_* of aslam_core.h
constexpr int SNAP_KNOWN_FLAGS = FLAG_INIT_X | FLAG_INIT_Z;

struct SnapBlobHeader
{
        char magic[8];
        uint32_t version, filter, count, reserved;
        uint64_t total_bytes;
        uint8_t zero[32];
};
struct SnapRecHeader
{
        int32_t n, flags;
        uint32_t status;
        int32_t sens_n, wait_n, ld;
        uint32_t reserved[2];
        double A[2];
        uint8_t zero[16];
};
static_assert(sizeof(SnapBlobHeader) == 64 && sizeof(SnapRecHeader) == 64, "the format of include/aslam_snapshot.h");

/// one record of a launch: where it lies in the blob, which slot of the context it belongs to, and its sizes AS THE HOST VALIDATED THEM
/// (the kernels never take a size from the blob)
struct SnapDesc
{
        int64_t off;
        int32_t slot, n, sens_n, wait_n;
        int32_t pad[2];
};

/// the context side of a launch
struct SnapCtx
{
        int NP, max_obs, max_wait;
        double *X, *Z, *P, *A;
        int *n, *flags;
        uint32_t *status;
        float *sens;
        int *sens_n;
        float *wait_rb;
        uint32_t *wait_cnt;
        int *wait_n;
        double *innov;                       // [B][2] or null: the last-callback record, NaN for a restored slot
        char *clear[SNAP_CLEAR_MAX];         // scratch buffers unpack zeroes (null = unused) ...
        size_t clear_bytes[SNAP_CLEAR_MAX];  // ... and the bytes of one slot in each (multiples of 16)
};

inline int64_t snap_pad64(int64_t x)
{
        return (x + 63) & ~(int64_t)63;
}

inline int64_t snap_record_bytes(int n, int sens_n, int wait_n)
{
        if (n < 3 || !(n & 1) || sens_n < 0 || wait_n < 0)
                return -1;
        const int64_t ld = n + 1;
        return 64 + 8 * ld * (n + 2) + 8 * (int64_t)sens_n + 12 * (int64_t)wait_n;
}

/// null, or what is wrong with the blob header for a blob of `bytes` bytes; *table_end: the first byte behind the offset table
inline const char *snap_check_header(const SnapBlobHeader &h, int64_t bytes, int64_t *table_end)
{
        if (bytes < 64)
                return "blob shorter than its header";
        if (memcmp(h.magic, "ASLSNP01", 8) != 0)
                return "not a snapshot (magic)";
        if (h.version != SNAP_VERSION)
                return "unknown snapshot version";
        if (h.filter > 1)
                return "unknown filter kind";
        if (h.count > 0x7fffffffu)
                return "record count out of range";
        *table_end = 64 + snap_pad64(8 * (int64_t)h.count);
        if (h.total_bytes > (uint64_t)bytes)
                return "blob truncated (total_bytes beyond the bytes given)";
        if ((int64_t)h.total_bytes < *table_end)
                return "offset table beyond total_bytes";
        return nullptr;
}

/// null, or what is wrong with record header r found at the (checked) offset `off` of a blob of `total` bytes
inline const char *snap_check_record(const SnapRecHeader &r, uint64_t off, uint64_t total)
{
        if (r.n < 3 || !(r.n & 1))
                return "state dimension is not 3 + 2k";
        if (r.ld != r.n + 1)
                return "ld is not n + 1";
        if (r.sens_n < 0 || r.wait_n < 0)
                return "negative count";
        if (r.flags & ~SNAP_KNOWN_FLAGS)
                return "unknown flag bit";
        if (r.status & ~SNAP_KNOWN_STATUS)
                return "unknown status bit";
        // (n <= 2^20 keeps the byte count far inside 64 bits; such a record would hold 8 TB)
        if (r.n > (1 << 20) || off + (uint64_t)snap_record_bytes(r.n, r.sens_n, r.wait_n) > total)
                return "record reaches beyond the blob";
        return nullptr;
}

/// null, or what is wrong with an offset (before the record header behind it is read)
inline const char *snap_check_offset(uint64_t off, int64_t table_end, uint64_t total)
{
        if (off & 63)
                return "record offset is not 64-byte aligned";
        if (off < (uint64_t)table_end || total < 64 || off > total - 64)
                return "record offset outside the blob";
        return nullptr;
}

// ---- device --------------------------------------------------------------------------------------------------------

/// Everything of record f that is not X, Z or P (the lists, the zero tail, both headers, the table entry), for every kernel that writes records;
/// called by all lanes of workgroup 0 of the record.  This function and snapshot_unpack are the two places that know the record format.
__device__ __forceinline__ void snap_write_lists_and_headers(const SnapCtx &c, const SnapDesc &d, int f, int count, uint32_t filter, uint64_t total,
                                                             char *rec, char *__restrict__ blob)
{
        const int tid = threadIdx.x;
        const int n = d.n, ld = n + 1;
        const size_t slot = (size_t)d.slot;
        float *sens = reinterpret_cast<float *>(rec + 64 + 8 * (size_t)ld * (n + 2));
        float *wrb = sens + 2 * d.sens_n;
        uint32_t *wcnt = reinterpret_cast<uint32_t *>(wrb + 2 * d.wait_n);
        for (int i = tid; i < 2 * d.sens_n; i += SNAP_WG)
                sens[i] = c.sens[slot * c.max_obs * 2 + i];
        for (int i = tid; i < 2 * d.wait_n; i += SNAP_WG)
                wrb[i] = c.wait_rb[slot * c.max_wait * 2 + i];
        for (int i = tid; i < d.wait_n; i += SNAP_WG)
                wcnt[i] = c.wait_cnt[slot * c.max_wait + i];
        uint32_t *end = wcnt + d.wait_n; // (4-byte units: every section is a multiple of 4 bytes)
        const int tail = (int)((64 - (end - reinterpret_cast<uint32_t *>(rec)) * 4 % 64) % 64) / 4;
        for (int i = tid; i < tail; i += SNAP_WG) // the padding behind the record
                end[i] = 0u;
        if (tid == 0)
        {
                SnapRecHeader r = {};
                r.n = n;
                r.flags = c.flags[slot] & SNAP_KNOWN_FLAGS;
                r.status = c.status[slot];
                r.sens_n = d.sens_n;
                r.wait_n = d.wait_n;
                r.ld = ld;
                r.A[0] = c.A[2 * slot];
                r.A[1] = c.A[2 * slot + 1];
                *reinterpret_cast<SnapRecHeader *>(rec) = r;
                reinterpret_cast<uint64_t *>(blob + 64)[f] = (uint64_t)d.off;
        }
        if (f == 0 && tid == 64) // (the second wave of record 0's workgroup: the first one's lane 0 writes the record header)
        {
                SnapBlobHeader bh = {};
                const char m[8] = {'A', 'S', 'L', 'S', 'N', 'P', '0', '1'};
                for (int i = 0; i < 8; ++i)
                        bh.magic[i] = m[i];
                bh.version = SNAP_VERSION;
                bh.filter = filter;
                bh.count = (uint32_t)count;
                bh.total_bytes = total;
                *reinterpret_cast<SnapBlobHeader *>(blob) = bh;
                for (int i = count; i & 7; ++i) // the table's padding to 64 bytes
                        reinterpret_cast<uint64_t *>(blob + 64)[i] = 0;
        }
}

/// One complete record per descriptor into `blob`.  Src, passed by value, says where X, Z and P come from: begin(c, d, f) is the per-record
/// setup (d.n: the dimension written), P(r, q) columns 2q, 2q + 1 of row r of P -- the last pair of a row is (P(r, n-1), 0) -- and XZ(z, q)
/// entries 2q, 2q + 1 of X (z = 0) or Z (z = 1), padded the same way.  The sources: SnapshotSrc below, PruneSrc (prune.h).
template <class Src>
__global__ __launch_bounds__(SNAP_WG) void record_pack(SnapCtx c, const SnapDesc *__restrict__ desc, int count, uint32_t filter, uint64_t total, Src src,
                                                       char *__restrict__ blob)
{
        const int tid = threadIdx.x;
        for (int f = blockIdx.y; f < count; f += gridDim.y)
        {
                const SnapDesc d = desc[f];
                const int n = d.n, ld = n + 1, h = ld / 2;
                src.begin(c, d, f);
                char *rec = blob + d.off;
                // P: n rows of ld, two doubles per access
                double2 *Pout = reinterpret_cast<double2 *>(rec + 64 + 16 * (size_t)ld);
                const int units = n * h;
                for (int i = blockIdx.x * SNAP_WG + tid; i < units; i += gridDim.x * SNAP_WG)
                {
                        const int r = i / h, q = i - r * h;
                        Pout[i] = src.P(r, q);
                }
                if (blockIdx.x != 0)
                        continue;
                // workgroup 0 of the record: X, Z, then everything else
                double2 *Xout = reinterpret_cast<double2 *>(rec + 64);
                for (int i = tid; i < 2 * h; i += SNAP_WG)
                        Xout[i] = src.XZ(i >= h, i < h ? i : i - h);
                snap_write_lists_and_headers(c, d, f, count, filter, total, rec, blob);
        }
}

/// the slot as it lies in the context: rows of stride NP, one 16-byte load per pair (NP is a multiple of 16)
struct SnapshotSrc
{
        const double *Pin, *Xin, *Zin; // the slot's P, X, Z
        size_t NP;
        int n;
        __device__ void begin(const SnapCtx &c, const SnapDesc &d, int)
        {
                NP = (size_t)c.NP, n = d.n;
                Pin = c.P + (size_t)d.slot * NP * NP, Xin = c.X + (size_t)d.slot * NP, Zin = c.Z + (size_t)d.slot * NP;
        }
        __device__ double2 pair(const double *p, int q) const
        {
                double2 v = *reinterpret_cast<const double2 *>(p + 2 * q);
                if (2 * q + 1 >= n)
                        v.y = 0.0;
                return v;
        }
        __device__ double2 P(int r, int q) const { return pair(Pin + (size_t)r * NP, q); }
        __device__ double2 XZ(int z, int q) const { return pair(z ? Zin : Xin, q); }
};

__global__ __launch_bounds__(SNAP_WG) void snapshot_unpack(SnapCtx c, const SnapDesc *__restrict__ desc, int count, const char *__restrict__ blob)
{
        const int tid = threadIdx.x;
        const size_t NP = (size_t)c.NP;
        const int h = c.NP / 2;
        const double2 zero2 = {0.0, 0.0};
        for (int f = blockIdx.y; f < count; f += gridDim.y)
        {
                const SnapDesc d = desc[f];
                const int n = d.n, ld = n + 1, lh = ld / 2;
                const size_t slot = (size_t)d.slot;
                const char *rec = blob + d.off;
                // the WHOLE padded P of the slot: rows and columns n .. NP-1 zero
                const double2 *Pin = reinterpret_cast<const double2 *>(rec + 64 + 16 * (size_t)ld);
                double2 *Pout = reinterpret_cast<double2 *>(c.P + slot * NP * NP);
                const int units = c.NP * h;
                for (int i = blockIdx.x * SNAP_WG + tid; i < units; i += gridDim.x * SNAP_WG)
                {
                        const int r = i / h, q = i - r * h;
                        double2 v = zero2;
                        if (r < n && 2 * q < n)
                        {
                                v = Pin[(size_t)r * lh + q];
                                if (2 * q + 1 >= n)
                                        v.y = 0.0;
                        }
                        Pout[i] = v;
                }
                // the slot's share of the scratch a reset zeroes
                for (int k = 0; k < SNAP_CLEAR_MAX; ++k)
                {
                        if (!c.clear[k])
                                continue;
                        double2 *p = reinterpret_cast<double2 *>(c.clear[k] + slot * c.clear_bytes[k]);
                        const size_t cu = c.clear_bytes[k] / 16;
                        for (size_t i = (size_t)blockIdx.x * SNAP_WG + tid; i < cu; i += (size_t)gridDim.x * SNAP_WG)
                                p[i] = zero2;
                }
                if (blockIdx.x != 0)
                        continue;
                const double2 *Xin = reinterpret_cast<const double2 *>(rec + 64);
                for (int i = tid; i < 2 * h; i += SNAP_WG)
                {
                        const int q = i < h ? i : i - h;
                        double2 v = zero2;
                        if (2 * q < n)
                        {
                                v = Xin[(i < h ? 0 : lh) + q];
                                if (2 * q + 1 >= n)
                                        v.y = 0.0;
                        }
                        *reinterpret_cast<double2 *>((i < h ? c.X : c.Z) + slot * NP + 2 * q) = v;
                }
                const float *sens = reinterpret_cast<const float *>(rec + 64 + 8 * (size_t)ld * (n + 2));
                const float *wrb = sens + 2 * d.sens_n;
                const uint32_t *wcnt = reinterpret_cast<const uint32_t *>(wrb + 2 * d.wait_n);
                for (int i = tid; i < 2 * c.max_obs; i += SNAP_WG)
                        c.sens[slot * c.max_obs * 2 + i] = i < 2 * d.sens_n ? sens[i] : 0.f;
                for (int i = tid; i < 2 * c.max_wait; i += SNAP_WG)
                        c.wait_rb[slot * c.max_wait * 2 + i] = i < 2 * d.wait_n ? wrb[i] : 0.f;
                for (int i = tid; i < c.max_wait; i += SNAP_WG)
                        c.wait_cnt[slot * c.max_wait + i] = i < d.wait_n ? wcnt[i] : 0u;
                if (tid == 0)
                {
                        const SnapRecHeader r = *reinterpret_cast<const SnapRecHeader *>(rec);
                        c.n[slot] = n;
                        c.flags[slot] = r.flags & SNAP_KNOWN_FLAGS;
                        c.status[slot] = r.status & SNAP_KNOWN_STATUS;
                        c.sens_n[slot] = d.sens_n;
                        c.wait_n[slot] = d.wait_n;
                        c.A[2 * slot] = r.A[0];
                        c.A[2 * slot + 1] = r.A[1];
                        if (c.innov)
                                c.innov[2 * slot] = c.innov[2 * slot + 1] = __builtin_nan("");
                }
        }
}

/// record header i of a device blob -> out[i]; `off`: the offset table AS THE HOST VALIDATED IT (a device copy of it)
__global__ __launch_bounds__(SNAP_WG) void snapshot_gather(const char *__restrict__ blob, const uint64_t *__restrict__ off, int count,
                                                           SnapRecHeader *__restrict__ out)
{
        const int i = blockIdx.x * SNAP_WG + threadIdx.x; // 16 bytes each: four lanes per header
        if (i < 4 * count)
                reinterpret_cast<uint4 *>(out)[i] = reinterpret_cast<const uint4 *>(blob + off[i >> 2])[i & 3];
}

/// n, the init flags and the list sizes of a filter, for the host: what a call needs to know of the batch before it can describe records
struct FilterMeta
{
        int32_t n, flags, sens_n, wait_n;
};

/// lanes over filters: the batch's FilterMeta into one array, for one copy to the host
__global__ __launch_bounds__(64) void filter_meta(const int *__restrict__ n, const int *__restrict__ flags, const int *__restrict__ sens_n,
                                                  const int *__restrict__ wait_n, int B, FilterMeta *__restrict__ meta)
{
        const int b = blockIdx.x * 64 + threadIdx.x;
        if (b < B)
                meta[b] = FilterMeta{n[b], flags[b], sens_n[b], wait_n[b]};
}

/// grid of a pack / unpack launch: `units` 16-byte accesses of the largest record, four per lane
inline dim3 snap_grid(int64_t units, int count)
{
        const int y = count < SNAP_GRID_CAP ? count : SNAP_GRID_CAP;
        int64_t x = (units + 4 * SNAP_WG - 1) / (4 * SNAP_WG);
        const int cap = SNAP_GRID_CAP / y;
        x = x < 1 ? 1 : x > cap ? cap : x;
        return dim3((unsigned)x, (unsigned)y);
}
} // namespace aslam
