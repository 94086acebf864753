// eks_prune.hpp -- launch interface of landmark evidence and the removal of
// landmarks from an associating EKF-SLAM handle (eks_prune.hip),
// used by ekf_api.hip.
#pragma once

#include "common.hpp"

namespace slam {

constexpr int kEksEvThreads = 1024;      // the evidence kernel's one workgroup (eks_assign_kernel's shape)
constexpr int kEksColThreads = 256;      // column pass: lanes of a row's workgroup
constexpr int kEksColUnroll = 8;         // ... elements per lane and chunk
constexpr int kEksColChunk = kEksColThreads * kEksColUnroll;   // 2,048 columns read, barrier, written
constexpr int kEksRowStrip = 16;         // row pass: columns of a wave's strip (one 128-byte line of a row)
constexpr int kEksRowBatch = 16;         // ... loads in flight per lane (4 rows each: 64 rows a batch)

// eks_evidence_kernel's result words (int32, read back by the host)
enum { kEksPrCount = 0, kEksPrRemoved = 1, kEksPrMoved = 2, kEksPrFirst = 3, kEksPrWords = 4 };

struct EksPrune {
    double vr2, view_tan;       // view_range^2; in view iff ry >= |rx| view_tan (with the angle)
    int32_t init, hit, miss, ev_max, remove_below;
};

// The evidence rule over the slots j < count (mu: the posterior state; taken:
// the assign kernel's marks over j < count0, NULL when nothing was matched),
// the compacted evidence in place, src[w] = the old slot of new slot w and the
// result words.
void eks_evidence_launch(hipStream_t stream, bool use_angle, const double* mu, int32_t count0,
                         int32_t count, const int32_t* taken, const EksPrune& P, int32_t* ev,
                         int32_t* src, int32_t* res);

// The same scan and outputs with the keep flags given: slot j < count is removed
// iff mask[j] != 0; ev may be NULL (a handle that does not prune).
void eks_mask_launch(hipStream_t stream, const int32_t* mask, int32_t count, int32_t* ev,
                     int32_t* src, int32_t* res);

// mu and the lower triangle of P (row-major, pitch ld) through src, in place:
// new slot w < count_new takes old slot src[w]; slots below first keep their
// place.  Three launches: columns within rows (and mu), rows, the vacated tail
// to zero.
void eks_compact_launch(hipStream_t stream, double* P, int64_t ld, double* mu, const int32_t* src,
                        int32_t first, int32_t count_new, int32_t count_old);

}  // namespace slam
