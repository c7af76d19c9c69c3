// fqd_sizein_core.hpp — the rules of FQD_FAST_SIZEIN: which bytes of a record's ID line are a `;size=N` annotation that the
// input already carries, the weight it gives the record, how the weights of a cluster add up, and how the new label takes
// the old annotation's place in a written record.  Shared by the device code (csrc/fqd_sizein.hip) and a CPU harness of the
// tests (tests/native/sizein_check.cpp builds this header with g++ and the sanitizers).
//
// ---- the annotation ---------------------------------------------------------------------------------------------------
// W          fqd_size_core.hpp's first word: the bytes of the ID line behind position 0 ('@' / '>') up to, not including, the
//            first of ' ', '\t', '\r', '\n' (the line's end where none occurs); wend = its end's position.  Nothing behind W
//            is looked at.
// candidate  a position p >= 1 with p + 6 <= wend at which the six bytes `;size=` stand, compared exactly.
// digits     the decimal digits that follow a candidate, p + 6 onward, inside W; they are looked at up to the ELEVENTH, so
//            nd = their number is 0 .. 11, 11 standing for "more than ten".
// end        what stands behind the digits (for nd <= 10): W's end, a ';', or another byte.
// The record's verdict, from the FIRST candidate from the left (none: weight 1, label_at = wend, cut = 0), is the first of
// these that holds:
//   kNoDigits  nd = 0                          kZero      the value is 0
//   kTooLarge  nd = 11                         kTooLarge  the value is above 2^31-1
//   kBadEnd    the end is another byte         kTwice     a second candidate stands in W
// and otherwise weight = the value, label_at = p, cut = 6 + nd: the annotation is the bytes [p, p + cut), a ';' behind it
// stays part of the record.  (So eleven digits or more are kTooLarge whatever follows them: no lane looks further.)
// Leading zeros count as digits.  In a paired run file 2's line is parsed by the same rule and an annotation there (cut > 0)
// must say file 1's weight: kMatesDiffer otherwise; none in file 2 is fine.
// None of the six bytes is a word end, so "p + 6 <= wend" is the same as "p < wend, p + 6 <= the line's length and the
// six bytes match": a lane that has not seen the word's end yet may test a candidate against the line's length alone.
//
// ---- sixteen lanes a record (csrc/fqd_sizein.hip; tests/native/sizein_check.cpp plays the lanes one after another) ---------
// rounds  fqd_umi_core.hpp's lane_look with ';' for the separator: lane gl holds the ';' of its sixteen bytes as a mask.  A ';'
//         is rare, so the lane tests each of its own for the five bytes behind it with byte loads (lane_candidates): a pattern
//         that straddles the lane's chunk or the group's 256-byte round is read where it lies, never beyond the line.  The
//         group takes the minimum of the lanes' first candidates and the sum of their counts; rounds go on until one holds
//         the word's end, as in size_labels_kernel.
// digits  lane gl < 11 looks at byte p + 6 + gl (lane_digit: a digit, a ';', another byte, or behind W); the classes come
//         together through ballots, nd = the ones below the first zero of the digit mask, the end is lane nd's class, and the
//         value is the sum over the lanes below nd of digit * 10^(nd - 1 - gl) in 64 bits (below 10^10).
//
// ---- the weighted run-length pass: a segmented sum in fqd_size_core.hpp's three launches ------------------------------------
// An element is a Seg (head, sum): head = "the last head place at or in front", kNone for none; sum = the weights since that
// head, its own included, in 64 bits.  Place k is (k where head[k] else kNone, weight[perm[k]]).
//   combine((p1, s1), (p2, s2)) = (p1, s1 + s2) if p2 == kNone, else (p2, s2).
// Associative — write a, b, c for three elements:
//   c.head != kNone:  (a∘b)∘c = c, and b∘c = c so a∘(b∘c) = a∘c = c.
//   c.head == kNone, b.head != kNone:  a∘b = b, so (a∘b)∘c = (b.head, b.sum + c.sum); b∘c is that same element, whose head
//                     is set, so a∘(b∘c) is it as well.
//   both kNone:       both sides are (a.head, a.sum + b.sum + c.sum); addition modulo 2^64 is associative.
// Identity (kNone, 0): x∘id = (x.head, x.sum + 0) = x; id∘x = (kNone, 0 + x.sum) = x where x.head is kNone, x otherwise.
// So combine(v(0), .., v(k)) = (start(k), the weights of places start(k) .. k), tile values and their exclusive combine carry
// a run across tiles exactly as fqd_size_core.hpp's max-scan does — a tile without a head has head kNone and passes the
// carry's head on with its weights added — and the last place of a run holds the run's whole sum.  n < 2^31 weights below
// 2^31 stay below 2^62: no sum wraps.  Who writes which entry of size is fqd_size_core.hpp's: every entry exactly once.
//
// ---- the label replaces the annotation: the spans still tile the output ------------------------------------------------------
// out_size[r] = rec_size[r] - cut[r] + label_len(size[r]) where keep[r], rec_size[r] elsewhere.  A span of grown length
// len = rec - cut + lab holds, for d in [0, len) (relabel_source): record byte d for d < at, label byte d - at for
// d < at + lab, record byte d - lab + cut behind it.  The record bytes taken are [0, at) and [at + cut, rec): d - lab + cut
// runs from at + cut (d = at + lab) to rec - 1 (d = len - 1), each once and in order.  So the span is the record without
// its annotation's cut bytes and with the label's lab bytes in their place, its length is exactly len, the three
// destination ranges [0, at), [at, at + lab), [at + lab, len) do not overlap, and the spans tile the output that
// fqd_output_plan summed from out_size.  cut = 0 is fqd_size_core.hpp's copy_source.
#pragma once
#include <cstdint>

#include "fqd_size_core.hpp"

#if defined(__HIPCC__)
#define FQD_SIZEIN_HD __host__ __device__ __forceinline__
#else
#define FQD_SIZEIN_HD inline
#endif

namespace fqdsizein {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kPattern = 6;                             // ";size="
constexpr uint32_t kMaxDigits = 10;
constexpr uint32_t kLookLanes = kMaxDigits + 1;              // the lanes that look at a digit place
constexpr uint32_t kMaxWeight = 0x7FFFFFFFu;

enum Reason : uint32_t { kOk = 0, kNoDigits = 1, kBadEnd = 2, kZero = 3, kTooLarge = 4, kTwice = 5, kMatesDiffer = 6 };
enum Class : uint32_t { kBehind = 0, kDigit = 1, kSemi = 2, kOther = 3 };      // what stands at a digit place (kBehind: W has ended)

struct Parsed { uint32_t weight, label_at, cut, reason; };

// Do the six bytes stand at p?  len = the line's length (or W's end: see the head of the file).
FQD_SIZEIN_HD bool candidate_at(const uint8_t* line, uint32_t len, uint32_t p)
{
    if (p < 1u || p > len || len - p < kPattern) return false;
    return line[p] == ';' && line[p + 1] == 's' && line[p + 2] == 'i' && line[p + 3] == 'z' && line[p + 4] == 'e' && line[p + 5] == '=';
}

FQD_SIZEIN_HD uint32_t classify(uint8_t b) { return b >= '0' && b <= '9' ? kDigit : b == ';' ? kSemi : kOther; }

// The verdict from what was found: count candidates, the first at `first`, nd digits of `value` behind it, `end` behind them.
FQD_SIZEIN_HD Parsed judge(uint32_t count, uint32_t first, uint32_t wend, uint32_t nd, uint32_t end, uint64_t value)
{
    if (count == 0) return Parsed{1u, wend, 0u, kOk};
    uint32_t reason = kOk;
    if (nd == 0) reason = kNoDigits;
    else if (nd > kMaxDigits) reason = kTooLarge;
    else if (end == kOther) reason = kBadEnd;
    else if (value == 0) reason = kZero;
    else if (value > kMaxWeight) reason = kTooLarge;
    else if (count > 1u) reason = kTwice;
    return Parsed{reason ? 1u : uint32_t(value), first, kPattern + (nd > kMaxDigits ? kMaxDigits : nd), reason};
}

// ---- the rule record by record ---------------------------------------------------------------------------------------------

FQD_SIZEIN_HD Parsed parse(const uint8_t* line, uint32_t len)
{
    const uint32_t wend = fqdsize::first_word_end(line, len);
    uint32_t first = kNone, count = 0;
    for (uint32_t p = 1; p + kPattern <= wend; ++p)
        if (candidate_at(line, wend, p)) { if (first == kNone) first = p; ++count; }
    if (!count) return judge(0u, kNone, wend, 0u, kBehind, 0u);
    uint32_t nd = 0;
    uint64_t value = 0;
    while (nd < kLookLanes && first + kPattern + nd < wend && classify(line[first + kPattern + nd]) == kDigit) {
        value = value * 10u + uint64_t(line[first + kPattern + nd] - '0');
        ++nd;
    }
    const uint32_t q = first + kPattern + nd;
    const uint32_t end = q < wend ? classify(line[q]) : uint32_t(kBehind);
    return judge(count, first, wend, nd, end, value);
}

// ---- the lanes' shares -------------------------------------------------------------------------------------------------------

struct Cand { uint32_t first, count; };

// Lane gl's candidates of one round: those of the ';' in its look k (fqdumi::lane_look with ';') that stand in front of `end`,
// the word's end as far as the group has seen it (kNone: not yet).  Every load lies inside the line.
FQD_SIZEIN_HD Cand lane_candidates(const uint8_t* line, uint32_t len, const fqdumi::Look& k, uint32_t end)
{
    Cand c{kNone, 0u};
    for (uint32_t m = k.seps; m; m &= m - 1u) {
        const uint32_t p = k.base + uint32_t(__builtin_ctz(m));
        if (p < end && candidate_at(line, len, p)) { if (c.first == kNone) c.first = p; ++c.count; }
    }
    return c;
}

// What lane gl sees at its digit place behind the candidate at `first` (kNone: there is none), and the digit's value.
FQD_SIZEIN_HD uint32_t lane_digit(const uint8_t* line, uint32_t wend, uint32_t first, uint32_t gl, uint32_t* digit)
{
    *digit = 0;
    if (first == kNone || gl >= kLookLanes) return kBehind;
    const uint32_t q = first + kPattern + gl;
    if (q >= wend) return kBehind;
    const uint8_t b = line[q];
    const uint32_t c = classify(b);
    if (c == kDigit) *digit = uint32_t(b - '0');
    return c;
}

// nd from the mask of the lanes that see a digit (bit gl = lane gl; lanes from kLookLanes on never do).
FQD_SIZEIN_HD uint32_t digits_in_front(uint32_t digit_mask) { return uint32_t(__builtin_ctz(~digit_mask)); }

// Lane gl's share of the value of nd <= 10 digits.
FQD_SIZEIN_HD uint64_t lane_value(uint32_t digit, uint32_t gl, uint32_t nd)
{
    if (nd > kMaxDigits || gl >= nd) return 0;
    uint64_t v = digit;
    for (uint32_t k = gl + 1u; k < nd; ++k) v *= 10u;
    return v;
}

// ---- the weighted run-length pass ----------------------------------------------------------------------------------------------

struct Seg { uint64_t sum; uint32_t head, pad; };            // 16 bytes a tile of scratch

FQD_SIZEIN_HD Seg seg_none() { return Seg{0u, kNone, 0u}; }
FQD_SIZEIN_HD Seg seg_of(bool head, uint32_t place, uint32_t weight) { return Seg{weight, head ? place : kNone, 0u}; }
FQD_SIZEIN_HD Seg combine(const Seg& a, const Seg& b) { return b.head == kNone ? Seg{a.sum + b.sum, a.head, 0u} : b; }

// ---- the copy ------------------------------------------------------------------------------------------------------------------

// Which byte destination byte d of a relabelled span is (fqdsize::Source); lab = label_len(size).
FQD_SIZEIN_HD fqdsize::Source relabel_source(uint32_t d, uint32_t at, uint32_t cut, uint32_t lab)
{
    if (d < at) return fqdsize::Source{false, d};
    if (d < at + lab) return fqdsize::Source{true, d - at};
    return fqdsize::Source{false, d - lab + cut};
}

FQD_SIZEIN_HD uint32_t relabelled_len(uint32_t rec, uint32_t cut, uint32_t size) { return rec - cut + fqdsize::label_len(size); }

// Lane l's share of a relabelled span: dst[0 .. len) from the record src[0 .. len - label_len(size) + cut), the label at
// label_at and the cut bytes behind label_at left out (len = the grown length; a label_at beyond what is left of the record
// is taken as its end, a len that cannot hold the label writes nothing).  Both parts by fqdsize::copy_part_lane; the last
// lane writes the label.
FQD_SIZEIN_HD void copy_relabelled_lane(const uint8_t* src, uint8_t* dst, uint32_t len, uint32_t label_at, uint32_t cut, uint32_t size, uint32_t l)
{
    const uint32_t lab = fqdsize::label_len(size);
    if (len < lab) return;
    const uint32_t kept = len - lab, at = label_at < kept ? label_at : kept;      // kept = the record's bytes that stay
    fqdsize::copy_part_lane(src, dst, at, l);
    fqdsize::copy_part_lane(src + at + cut, dst + at + lab, kept - at, l);
    if (l == fqdsize::kSpanLanes - 1u) {
        uint8_t text[fqdsize::kMaxLabel];
        const uint32_t got = fqdsize::write_label(text, size);
        for (uint32_t k = 0; k < got; ++k) dst[at + k] = text[k];
    }
}

} // namespace fqdsizein
