// fqd_size_core.hpp — the rules of FQD_FAST_SIZEOUT / FQD_FAST_LEVELS: how many members every cluster of the `--fast` mode
// has, the `;size=N` label a written record carries, and the duplication level a cluster counts in.  Shared by the device
// code (csrc/fqd_size.hip) and a CPU harness of the tests (tests/native/size_check.cpp builds this header with g++ and the
// sanitizers).
//
// ---- definitions ------------------------------------------------------------------------------------------------------
// (perm, head)  an order of the n records (pairs) and a flag at the first place of every cluster: fqd_group_owners', after
//               the optional pick (fqd_seq_pick_best), so that perm[k] at a head's place k is the record that is written.
//               head[0] = 1; n < 2^31.
// run           the places s .. e-1 with head[s] set, head[s+1 .. e-1] clear and (e = n or head[e] set).
// start(k)      the s of the run that holds place k = max { j <= k : head[j] }.
// size[r]       e - s for r = perm[s] of a run; 0 for every other record.
// level(N)      the row of `<output>.duplevels` a cluster of N members counts in: 1 .. 9 one row each, then 10-49, 50-99,
//               100-499, 500-999, 1000-4999, 5000-9999, 10000+: sixteen rows.
// label(N)      ";size=" and N in decimal, no padding: label_len(N) = 6 + digits(N) bytes.
// label_at      where the label goes into a record: the length of '@' / '>' and the first word of its ID line, which ends
//               in front of the first ' ', '\t', '\r' or '\n' behind position 0 (fqd_umi_core.hpp's W); the line's length
//               where it holds none.  A `;size=` that the line already holds is not looked at.
//
// ---- the run-length pass: a max-scan in three launches (the scan shape of fqd_record_scan.hpp) ------------------------------
// v(j) = j where head[j], kNone elsewhere; combine(a, b) = the larger of the two, kNone standing for "no head yet" (it is
// the identity: combine(kNone, x) = combine(x, kNone) = x).  combine is associative and start(k) = combine(v(0), .., v(k)).
//   tiles   launch 1: T(t) = combine over the places of tile t (kOffTile places a block).
//   carry   launch 2, one block: C(t) = combine(T(0), .., T(t-1)), kNone for t = 0.
//   places  launch 3: start(k) = combine(C(t), v(first place of t), .., v(k)).
// A run that spans tiles gets its start from the tiles in front: a tile without a head has T(t) = kNone, the identity, so
// C(t+1) = C(t) passes through it unchanged, and a place in front of its tile's first head combines C(t) with kNone's only:
// start(k) = C(t) = the last head of all tiles in front, which exists because head[0] is set.  No block waits for another:
// each launch reads what the launch before it has finished.
//
// ---- every entry of size is written exactly once ---------------------------------------------------------------------------
// Place k writes size[perm[k]] = 0 unless head[k]; the LAST place of a run (k = n-1 or head[k+1]) writes
// size[perm[start(k)]] = k + 1 - start(k).  Every place belongs to exactly one run and every run has exactly one head place
// and one last place (which may be the same: a singleton, whose one place writes the 1).  So the head place of a run is
// written once, by the run's last place, and every other place once, by itself; perm is a permutation, so these are n
// writes to n different entries: no atomics, no order between them.
//
// ---- out_size sums to the output's size ------------------------------------------------------------------------------------
// out_size[r] = rec_size[r] + label_len(size[r]) where keep[r], rec_size[r] elsewhere.  fqd_output_plan sums it over the
// kept records: the sum of their sizes, which is the unlabelled output, plus one label each.  A labelled span of grown
// length len holds, for d in [0, len) (copy_source): the record's byte d in front of label_at, the label's byte
// d - label_at for the next label_len bytes, the record's byte d - label_len behind it — the record's len - label_len
// bytes, each once and in order, around the label.  So the spans tile the output exactly and the text without its labels
// is the default run's.
//
// ---- eight lanes a span (csrc/fqd_size.hip; tests/native/size_check.cpp plays the lanes one after another) -----------------
// copy_labelled_lane is fqd_copy_spans' rule applied to the two parts on their own: a part of sixteen bytes or more goes in
// 16-byte moves, lane l taking chunks l, l + 8, .., and when its length is no multiple of sixteen its last sixteen bytes once
// more (the same bytes to the same place); a shorter part goes byte by byte.  Every load lies inside the part's source,
// every store inside its destination, and the two destinations and the label's do not overlap.  One lane writes the label.
#pragma once
#include <cstdint>

#include "fqd_umi_core.hpp"                                  // is_word_end: the first word is that header's W

#if defined(__HIPCC__)
#define FQD_SIZE_HD __host__ __device__ __forceinline__
#else
#define FQD_SIZE_HD inline
#endif

namespace fqdsize {

constexpr uint32_t kLevels = 16;
constexpr uint32_t kNone = 0xFFFFFFFFu;                      // "no head at or in front of here": the scan's identity
constexpr uint32_t kSpanLanes = 8;                           // lanes a span (fqd_copy_spans' shape)
constexpr uint32_t kLabelHead = 6;                           // ";size="
constexpr uint32_t kMaxLabel = kLabelHead + 10;              // 4294967295 has ten digits

// The row a cluster of `size` members counts in (size >= 1).
FQD_SIZE_HD uint32_t level(uint32_t size)
{
    if (size < 10u) return size ? size - 1u : 0u;
    if (size < 50u) return 9u;
    if (size < 100u) return 10u;
    if (size < 500u) return 11u;
    if (size < 1000u) return 12u;
    if (size < 5000u) return 13u;
    if (size < 10000u) return 14u;
    return 15u;
}

FQD_SIZE_HD uint32_t digits(uint32_t v)
{
    uint32_t d = 1;
    while (v >= 10u) { v /= 10u; ++d; }
    return d;
}

FQD_SIZE_HD uint32_t label_len(uint32_t size) { return kLabelHead + digits(size); }

// dst[0 .. label_len(size)) = ";size=<size>"; returns label_len(size).
FQD_SIZE_HD uint32_t write_label(uint8_t* dst, uint32_t size)
{
    const char head[kLabelHead + 1] = ";size=";
    for (uint32_t k = 0; k < kLabelHead; ++k) dst[k] = uint8_t(head[k]);
    const uint32_t d = digits(size);
    for (uint32_t k = d; k > 0; --k) { dst[kLabelHead + k - 1u] = uint8_t('0' + size % 10u); size /= 10u; }
    return kLabelHead + d;
}

// The scan's combine: the later head of the two, kNone being none.
FQD_SIZE_HD uint32_t combine(uint32_t a, uint32_t b) { return a == kNone ? b : b == kNone ? a : (a > b ? a : b); }

// label_at of a line of len bytes: the position of the first word end behind position 0, len for none.
FQD_SIZE_HD uint32_t first_word_end(const uint8_t* line, uint32_t len)
{
    for (uint32_t i = 1; i < len; ++i)
        if (fqdumi::is_word_end(line[i])) return i;
    return len;
}

// Which byte destination byte d of a labelled span is: a byte of the label (at = its index in the label) or of the record
// (at = its index in the record).  lab = label_len(size).
struct Source { bool label; uint32_t at; };
FQD_SIZE_HD Source copy_source(uint32_t d, uint32_t label_at, uint32_t lab)
{
    if (d < label_at) return Source{false, d};
    if (d < label_at + lab) return Source{true, d - label_at};
    return Source{false, d - lab};
}

// Lane l's share of b[0 .. L) = a[0 .. L): fqd_copy_spans' rule for one part.
FQD_SIZE_HD void copy_part_lane(const uint8_t* a, uint8_t* b, uint32_t L, uint32_t l)
{
    if (L < 16u) { for (uint32_t k = l; k < L; k += kSpanLanes) b[k] = a[k]; return; }
    for (uint32_t k = 16u * l; k + 16u <= L; k += 16u * kSpanLanes) {
        uint64_t w[2];
        __builtin_memcpy(w, a + k, 16);
        __builtin_memcpy(b + k, w, 16);
    }
    if ((L & 15u) && l == ((L / 16u) % kSpanLanes)) {        // (the lane whose turn the next chunk would have been)
        uint64_t w[2];
        __builtin_memcpy(w, a + L - 16u, 16);
        __builtin_memcpy(b + L - 16u, w, 16);
    }
}

// Lane l's share of a labelled span: dst[0 .. len) from the record src[0 .. len - label_len(size)) and the label at label_at
// (len = the grown length; a label_at beyond the record is taken as the record's end, a len that cannot hold the label writes
// nothing).  The last lane writes the label: with spans of a few hundred bytes it is the one with the fewest chunks.
FQD_SIZE_HD void copy_labelled_lane(const uint8_t* src, uint8_t* dst, uint32_t len, uint32_t label_at, uint32_t size, uint32_t l)
{
    const uint32_t lab = label_len(size);
    if (len < lab) return;
    const uint32_t rec = len - lab, at = label_at < rec ? label_at : rec;
    copy_part_lane(src, dst, at, l);
    copy_part_lane(src + at, dst + at + lab, rec - at, l);
    if (l == kSpanLanes - 1u) {
        uint8_t text[kMaxLabel];
        const uint32_t got = write_label(text, size);
        for (uint32_t k = 0; k < got; ++k) dst[at + k] = text[k];
    }
}

} // namespace fqdsize
