// csrc/sepaihrd_mh_layout.h -- the layout of every slab the device-resident sampler (csrc/sepaihrd_mh_capi.cpp) carves into
// several arrays: ONE statement of each slab's size and offsets, and a view struct whose members are the arrays.  A slab is
// one allocation on the device and one page-locked mirror of the same layout, so that one copy moves it; a view's first
// member is the slab's base.  Host code only, no HIP: C chains, P parameters.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace sepaihrd {
namespace mh_layout {

constexpr size_t up8(size_t v) { return (v + 7) & ~(size_t)7; }
template <class T>
T* at(void* slab, size_t byte_offset) { return reinterpret_cast<T*>(static_cast<char*>(slab) + byte_offset); }

// ---- the packed upload of sepaihrd_mh_step: [accept C bytes | pad to 8 | scale C doubles | chain C int32 | pad to 8 | rows C*P doubles]
// chain / rows: the n_patch chains whose normals were drawn again, and their rows
struct Pack { uint8_t* accept; double* scale; int32_t* chain; double* rows; };
constexpr size_t pack_off_scale(size_t C) { return up8(C); }
constexpr size_t pack_off_chain(size_t C) { return pack_off_scale(C) + C * sizeof(double); }
constexpr size_t pack_off_rows(size_t C) { return up8(pack_off_chain(C) + C * sizeof(int32_t)); }
constexpr size_t pack_bytes(size_t C, size_t P) { return pack_off_rows(C) + C * P * sizeof(double); }
// what one step sends: up to the end of the scales when nothing is patched, else up to the last patched row
constexpr size_t pack_sent_bytes(size_t C, size_t P, size_t n_patch) {
    return n_patch > 0 ? pack_off_rows(C) + n_patch * P * sizeof(double) : pack_off_chain(C);
}
inline Pack pack_view(void* slab, size_t C) {
    return Pack{at<uint8_t>(slab, 0), at<double>(slab, pack_off_scale(C)), at<int32_t>(slab, pack_off_chain(C)), at<double>(slab, pack_off_rows(C))};
}

// ---- the accept test's inputs: [log_u C][scale_reject C][scale_accept C][z_plain C*P], doubles
struct TestInputs { double* log_u; double* scale_reject; double* scale_accept; double* z_plain; };
constexpr size_t test_inputs_doubles(size_t C, size_t P) { return 3 * C + C * P; }
constexpr size_t test_inputs_bytes(size_t C, size_t P) { return test_inputs_doubles(C, P) * sizeof(double); }
// what a caller who draws on the host sends (the last test has no proposal after it: no normals), and what one sends whose
// draws are the device's: the two scale candidates
constexpr size_t test_inputs_sent_bytes(size_t C, size_t P, bool with_normals) { return test_inputs_bytes(C, with_normals ? P : 0); }
constexpr size_t test_scales_bytes(size_t C) { return 2 * C * sizeof(double); }
inline TestInputs test_inputs_view(double* slab, size_t C) { return TestInputs{slab, slab + C, slab + 2 * C, slab + 3 * C}; }

// ---- the accept test's outcome: [values C doubles][flags C bytes]
struct TestOutcome { double* values; uint8_t* flags; };
constexpr size_t test_outcome_bytes(size_t C) { return C * (sizeof(double) + 1); }
inline TestOutcome test_outcome_view(void* slab, size_t C) { return TestOutcome{at<double>(slab, 0), at<uint8_t>(slab, C * sizeof(double))}; }

// ---- an evaluation's results as the sampler fetches them: [loglik C doubles][status C int32]
struct Fetch { double* loglik; int32_t* status; };
constexpr size_t fetch_bytes(size_t C, bool with_status = true) { return C * sizeof(double) + (with_status ? C * sizeof(int32_t) : 0); }
inline Fetch fetch_view(void* slab, size_t C) { return Fetch{at<double>(slab, 0), at<int32_t>(slab, C * sizeof(double))}; }

// ---- the queued rank-one updates, for a capacity of cap entries: [gammas cap doubles | rows cap int32], both aligned whatever
// the number n of entries in use
struct Rank1 { double* gammas; int32_t* rows; };
constexpr size_t rank1_bytes(size_t cap) { return cap * (sizeof(double) + sizeof(int32_t)); }
constexpr size_t rank1_sent_bytes(size_t cap, size_t n) { return cap * sizeof(double) + n * sizeof(int32_t); }
inline Rank1 rank1_view(void* slab, size_t cap) { return Rank1{at<double>(slab, 0), at<int32_t>(slab, cap * sizeof(double))}; }

// ---- a snapshot's record of one chain: [value, best, scale, accepted | samples count*P | sample values count], doubles
struct SnapshotRecord { const double* state; const double* samples; const double* sample_values; };
constexpr size_t snapshot_width(size_t P, size_t count) { return 4 + count * (P + 1); }
inline SnapshotRecord snapshot_record(const double* table, size_t k, size_t P, size_t count) {
    const double* o = table + k * snapshot_width(P, count);
    return SnapshotRecord{o, o + 4, o + 4 + count * P};
}

}  // namespace mh_layout
}  // namespace sepaihrd
