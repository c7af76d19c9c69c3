// fqd_bgzf_search_core.hpp — the second mode of the device deflater (FQD_BGZF_SEARCH): a real LZ77 search
// over the member.  Framing, Huffman codes, pricing, emission, CRC-32 and compaction are those of
// fqd_bgzf_core.hpp; what is new is where the tokens come from:
//   * a hash table over the member's kHashBytes-byte prefixes in LDS: kBuckets buckets of kWays positions each, the
//     most recent ones.  The member is walked in ROUNDS of kThreads consecutive positions, one per thread:
//     all of a round's positions are looked up (matches before the round), a barrier, all are inserted, a
//     barrier, all are looked up again (matches inside the round).  An insert is a cascade
//     of atomicMax down the ways of a bucket (a way keeps the larger value and hands the smaller one on), so
//     a bucket ends every round holding its kWays LARGEST positions whatever the order in which the threads
//     arrive — the GPU and the CPU run of these functions see the same table;
//   * a lookup takes the bucket's entries below its own position, nearest first, compares each over kProbe
//     bytes and extends the kDeep nearest that agree that far with word-wide compares; the longest wins, the
//     nearer one on a tie.  A match may READ from anywhere earlier
//     in the member (distance <= 32768) but is CUT at the end of the 128-byte chunk its position lies in:
//     chunks stay the unit of pricing and emission, as in the fast mode, so the two block scans, the bit
//     writers and the stored fallback are shared.  The result (length | distance << 8) of every position goes
//     to the workgroup's piece of the engine's scratch;
//   * every trip count is bounded by a constant: kWays entries a lookup, kDeep extensions of kChunk / 4 words,
//     kWays atomics an insert.  A member whose positions all hash alike costs what any other member costs;
//   * the parse of a chunk is the owning thread's, as before: at every position the hash candidate competes
//     with the two structural ones of the fast mode (run, column), and a match is put off by one position
//     when the next position holds a longer one (zlib's lazy evaluation, one step of look-ahead).
// Everything here is `FQD_HD` and runs unchanged in tests/native/bgzf_search_check.cpp.
#pragma once

#include "fqd_bgzf_core.hpp"

namespace fqd {
namespace bgzf {

constexpr uint32_t kEffortFast = 0, kEffortSearch = 1;
// The knobs can be set from the compiler's command line, for the CPU harness to price variants with.
#ifndef FQD_SEARCH_HASH_BITS
#define FQD_SEARCH_HASH_BITS 10
#endif
#ifndef FQD_SEARCH_WAYS
#define FQD_SEARCH_WAYS 16
#endif
#ifndef FQD_SEARCH_LAZY
#define FQD_SEARCH_LAZY 1
#endif
constexpr uint32_t kHashBits = FQD_SEARCH_HASH_BITS, kBuckets = 1u << kHashBits, kWays = FQD_SEARCH_WAYS;
#ifndef FQD_SEARCH_HASH_BYTES
#define FQD_SEARCH_HASH_BYTES 6
#endif
constexpr bool kLazy = FQD_SEARCH_LAZY != 0;
constexpr uint32_t kHashBytes = FQD_SEARCH_HASH_BYTES;               // 4..8: the prefix a position is filed under
constexpr uint32_t kMaxDistance = 32768;
#ifndef FQD_SEARCH_DEEP
#define FQD_SEARCH_DEEP 4
#endif
constexpr uint32_t kProbe = 8, kDeep = FQD_SEARCH_DEEP;            // lookup: bytes every entry is compared over; entries extended to the end
constexpr uint32_t kRounds = (kMember + kThreads - 1u) / kThreads;


// Four bytes from any position (the data types read words at multiples of four).
template <class Data>
FQD_HD uint32_t load4(const Data& data, uint32_t p)
{
    const uint32_t a = p & ~3u, sh = (p & 3u) * 8u;
    const uint32_t w0 = data.word(a);
    return sh ? (w0 >> sh) | (data.word(a + 4u) << (32u - sh)) : w0;
}

template <class Data>
FQD_HD uint32_t hash_at(const Data& data, uint32_t p)
{
    uint32_t w = load4(data, p) * 2654435761u;
    if (kHashBytes > 4u) w = (w ^ (load4(data, p + 4u) & (0xFFFFFFFFu >> (8u * (8u - kHashBytes))))) * 2246822519u;
    return w >> (32u - kHashBits);
}

// Inside a byte run (the byte before p and the kHashBytes from p on are one and the same byte) the table is left alone,
// both ways: the distance-1 candidate of the parse covers the run, and a quality line of one letter would otherwise
// send half of a member's positions through the atomics of ONE bucket.  p + kHashBytes <= L.
template <class Data>
FQD_HD bool inside_run(const Data& data, uint32_t p)
{
    if (p == 0u) return false;
    const uint32_t w = load4(data, p), b = w & 0xFFu;
    if (w != b * 0x01010101u || uint32_t(data[p - 1u]) != b) return false;
    return kHashBytes <= 4u || (load4(data, p + 4u) & (0xFFFFFFFFu >> (8u * (8u - kHashBytes)))) == ((b * 0x01010101u) & (0xFFFFFFFFu >> (8u * (8u - kHashBytes))));
}

// End of the chunk that position p of a member of L bytes lies in (chunks are right-aligned: chunk_of).
FQD_HD uint32_t chunk_end(uint32_t p, uint32_t L) { return L - ((L - 1u - p) / kChunk) * kChunk; }

// Position p into its bucket.  `max_into(ptr, v)` is atomicMax: it returns what was there.
template <class Data, class Max>
FQD_HD void search_insert(const Data& data, uint32_t* table, uint32_t p, uint32_t L, Max max_into)
{
    if (p + kHashBytes > L || inside_run(data, p)) return;
    uint32_t* bucket = table + hash_at(data, p);                     // way w of bucket h at w * kBuckets + h: see search_lookup
    uint32_t v = p + 1u;                                             // 0 = empty
#pragma unroll
    for (uint32_t w = 0; w < kWays; ++w) {
        const uint32_t old = max_into(bucket + w * kBuckets, v);
        v = old < v ? old : v;
        if (v == 0u) break;
    }
}

// Bytes that agree at p and q (q < p), at most `room`.
template <class Data>
FQD_HD uint32_t match_length(const Data& data, uint32_t p, uint32_t q, uint32_t room)
{
    uint32_t i = 0;
    for (uint32_t k = 0; k < kChunk / 4u && i < room; ++k) {         // room <= kChunk
        const uint32_t x = load4(data, p + i) ^ load4(data, q + i);
        if (x) { i += uint32_t(__builtin_ctz(x)) >> 3; break; }
        i += 4u;
    }
    return i < room ? i : room;
}

// The best match the table knows for position p among the positions in [from, p), or `prior` (an earlier answer for p)
// where that one is as long: length | distance << 8, 0 when there is none.  A round asks twice: before its inserts
// (the table holds what lies before the round: from = 0) and after them (from = the round's first position: the near
// matches, which would otherwise be missed, while the far ones may have been pushed out of a crowded bucket by now).
template <class Data>
FQD_HD uint32_t search_lookup(const Data& data, const uint32_t* table, uint32_t p, uint32_t L, uint32_t from, uint32_t prior)
{
    if (p + kHashBytes > L || inside_run(data, p)) return 0u;
    const uint32_t room = chunk_end(p, L) - p;
    if (room < kMinMatch) return 0u;
    // way-major: the lanes of a wave read way w of 64 buckets, which lie in as many banks as their hashes differ in the low
    // six bits (bucket-major, 16 words a bucket, they would share four banks)
    const uint32_t* bucket = table + hash_at(data, p);
    uint32_t best = prior & 0xFFu, dist = prior >> 8;
    // Two steps, so that the lanes of a wave stay together: every entry is compared over kProbe bytes (two words, whatever
    // the data), and only the kDeep nearest entries that agree that far are extended to the end — one lane on an ID
    // line would otherwise hold its wave in sixteen loops of thirty turns.
    const uint32_t probe = room < kProbe ? room : kProbe;
    uint32_t deep[kDeep], n_deep = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWays; ++w) {                           // descending: nearest first
        const uint32_t e = bucket[w * kBuckets];
        if (e == 0u) break;
        const uint32_t q = e - 1u;
        if (q >= p) continue;                                        // inserted in this round, at or after p
        const uint32_t d = p - q;
        if (d > kMaxDistance || q < from) break;
        const uint32_t len = match_length(data, p, q, probe);
        if (len == probe && probe < room) {
            if (n_deep < kDeep) {
#pragma unroll
                for (uint32_t k = 0; k < kDeep; ++k) if (k == n_deep) deep[k] = d;      // (no indexed registers)
                ++n_deep;
            }
        } else if (len > best || (len == best && d < dist)) { best = len; dist = d; }
    }
#pragma unroll
    for (uint32_t k = 0; k < kDeep; ++k) {
        if (k >= n_deep) break;
        const uint32_t len = match_length(data, p, p - deep[k], room);
        if (len > best || (len == best && deep[k] < dist)) { best = len; dist = deep[k]; }
    }
    if (best < kMinMatch) return 0u;
    return best | (dist << 8);
}

// The two structural candidates of the fast mode at offset p of the chunk (parse_chunk's choice).
FQD_HD void structural_at(const Scan& sc, const Columns& col, uint32_t p, uint32_t room, uint32_t& best, uint32_t& dist)
{
    best = 0; dist = 0;
    if (room < kMinMatch) return;
    if (bit_of(sc.eq, p)) {
        uint32_t r = run_from(sc.eq, p);
        r = r < room ? r : room;
        if (r >= kMinMatch) { best = r; dist = 1; }
    }
    if (bit_of(col.same, p) && best < room) {
        uint32_t r = run_from(col.same, p);
        r = r < room ? r : room;
        const bool first = p < col.split;
        if (first && r > col.split - p) r = col.split - p;
        if (r >= kMinMatch && r > best) { best = r; dist = first ? col.delta0 : col.delta1; }
    }
    if (bit_of(col.same_r, p) && best < room) {
        uint32_t r = run_from(col.same_r, p);
        r = r < room ? r : room;
        const bool first = p < col.split;
        if (first && r > col.split - p) r = col.split - p;
        if (r >= kMinMatch && r > best) { best = r; dist = first ? col.rdelta0 : col.rdelta1; }
    }
}

// Is a match worth its bits?  FASTQ literals are cheap (two to four bits), and a short match far back costs more
// than the literals it replaces: the match under the codes against the literals of its first bytes.  Which codes: the
// emit kernel has the call's own.  The histogram pass they are built from has none yet, and guessing there goes wrong
// both ways (count the matches of random bases and their symbols get the short codes, the bases the long ones, and the
// matches then ARE cheaper: 6 % larger than the fast mode on flat-quality text).  So the call is counted as the fast
// mode would parse it — literals at their cheapest — and then kSearchCounts times as the search parses it, each time
// under the codes of the count before: the codes and the parse settle on each other from the cheap-literal side.
// Measured with the CPU harness (mixed / binned / flat qualities, 20 000 records): one search count 2 299 621 /
// 1 728 106 / 1 036 578, two 2 180 055 / 1 725 103 / 1 036 826, three 2 168 349 / 1 725 103 / 1 037 193.
constexpr uint32_t kSearchCounts = 2;
constexpr uint32_t kWorthBytes = 12;                                 // longer matches are taken unseen
struct WorthCodes {
    const uint32_t* lit; const uint32_t* dst;
    template <class Data>
    FQD_HD bool operator()(const Data& data, uint32_t at, uint32_t len, uint32_t dist) const
    {
        if (len > kWorthBytes) return true;
        const Sym l = length_symbol(len), d = dist_symbol(dist);
        const uint32_t cost = (lit[l.sym] >> 16) + l.ebits + (dst[d.sym] >> 16) + d.ebits;
        uint32_t plain = 0;
        for (uint32_t i = 0; i < kWorthBytes; ++i) if (i < len) plain += lit[data[at + i]] >> 16;
        return cost < plain;
    }
};

// The best of all candidates at offset p of the chunk; found[] holds search_lookup's results of the chunk.
template <class Data, class Worth>
FQD_HD void candidate_at(const Data& data, uint32_t lo, const Worth& worth, const Scan& sc, const Columns& col, const uint32_t* found, uint32_t p, uint32_t L,
                         uint32_t& best, uint32_t& dist)
{
    structural_at(sc, col, p, L - p, best, dist);
    const uint32_t f = found[p], flen = f & 0xFFu, fdist = f >> 8;
    if (flen > best || (flen == best && flen && fdist < dist)) { best = flen; dist = fdist; }
    if (best && !worth(data, lo + p, best, dist)) best = 0;
}

// Parse of [lo, hi) with one position of look-ahead.  found = the search results of the member's position lo onwards.
template <class Data, class Worth, class Sink>
FQD_HD void parse_chunk_search(const Data& data, uint32_t lo, uint32_t hi, const Scan& sc, const Columns& col, const uint32_t* found,
                                const Worth& worth, Sink& sink)
{
    const uint32_t L = hi - lo;
    uint32_t p = 0, best = 0, dist = 0;
    if (L) candidate_at(data, lo, worth, sc, col, found, 0u, L, best, dist);
    while (p < L) {                                                  // every turn advances p
        uint32_t nbest = 0, ndist = 0;
        if (kLazy && p + 1u < L) candidate_at(data, lo, worth, sc, col, found, p + 1u, L, nbest, ndist);
        if (best && nbest <= best) {
            sink.match(best, dist);
            p += best;
            if (p < L) candidate_at(data, lo, worth, sc, col, found, p, L, best, dist);
        } else {
            sink.literal(data[lo + p]);
            ++p; best = nbest; dist = ndist;
            if (!kLazy && p < L) candidate_at(data, lo, worth, sc, col, found, p, L, best, dist);
        }
    }
}

} // namespace bgzf
} // namespace fqd
