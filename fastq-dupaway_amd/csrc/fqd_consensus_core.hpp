// fqd_consensus_core.hpp — the rule of FQD_FAST_CONSENSUS=1: what is written in place of the sequence and quality lines of a
// cluster's written member, so that a read with a sequencing error that happens to come first does not survive its correct
// copies.  Shared by the device code (csrc/fqd_consensus.hip) and a CPU harness of the tests (tests/native/consensus_check.cpp
// builds this header with g++ and the sanitizers); tests/consensus_reference.py states the same rule sequentially in Python.
//
// ---- a vote ---------------------------------------------------------------------------------------------------------------------
// cluster    a run of (perm, head) of fqd_group_owners; its written member is perm[head place].  A cluster of ONE member is not
//            touched.  Of a cluster of m >= 2 members each mate (file) is voted on its own; within a cluster all members have
//            one length L in a mate (the key, and the shape rule of fqd_near_core.hpp), and a record's quality line is as long
//            as its sequence line (the record scan), so the result has exactly the written member's length.
// column     position p < L of the mate.  Member i has the base b_i = seq_i[p] and the weight w_i: 0 where b_i is no A, C, G
//            or T, else q_i[p] - 33 for a quality byte of 33 or more and 0 for a byte below 33 (fqd_seq_pick_core.hpp's
//            convention for a quality byte).  A base byte that is none of A, C, G, T stands for N: it votes as N, with weight 0.
// S[x]       the sum of w_i over the members with letter x, for x in A, C, G, T, N (S[N] is always 0).
// present    a letter some member carries.  At least one is: m >= 1.
// winner     the present letter with the largest S.  Among tied letters the written member's letter wins if it is one of
//            them, otherwise the first in the order A, C, G, T, N.  N wins only where no other present letter has weight.
// quality    Q = S[winner] - (the sum of S over the other letters), clamped to 0 .. 93; the byte written is 33 + Q ('~' at
//            most).  Agreeing observations add their Phred scores, disagreeing ones take theirs away.
// written    the winner's letter where it is not the written member's own letter (a column that counts as changed; where it is,
//            the sequence byte stays as it is, also where it is a byte that only stands for N), and the quality byte, over all L
//            columns of the written member.  No other byte of the text changes.
//
// ---- the state of a column, and why any split of the members gives one result ---------------------------------------------------
// A column's state is (S[0..4], mask): five sums and the 5-bit set of present letters.  The state of the empty set of members
// is (0, 0, 0, 0, 0, 0); add() is the state of one member combined into another.
// combine(a, b) = (a.S[x] + b.S[x] for every x, a.mask | b.mask).
// (a) + on integers that do not overflow and | on bits are associative and commutative, and 0 is neutral for both; so combine
//     is associative and commutative with the empty state as its neutral element, component by component.
// (b) By induction on the number of members: the state of a set of members is the combine of the states of its members one by
//     one, in any order, and with (a) the combine of the states of the parts of ANY partition of the set, in any grouping
//     and order.  Lanes, waves and workgroups each hold a part; an atomic add / or into memory is combine with one part.  So the
//     state that decide() sees is a function of the SET of members alone: not of how they were dealt to lanes, waves or
//     workgroups, nor of the order in which atomics arrive.
// (c) decide() reads the state and the written member's own letter and nothing else, so the bytes written and the counts are
//     the same from run to run and from tier to tier.
// (d) No overflow.  A weight is at most 255 - 33 = 222 (93 for a valid Phred+33 byte).  Sum32 states hold at most kMax32
//     members' weights: 222 * 2^20 < 2^28.  The device uses Sum32 only for a set of members that its tier bounds to kMax32
//     (a lane group's cluster; a workgroup's cluster, or its share of a larger one) and Sum64 above: 222 * 2^31 < 2^39.
//     Q is computed in 64 bits signed: |S[w] - others| < 2^39.
#pragma once
#include <cstdint>

#include "fqd_seq_core.hpp"

namespace fqdconsensus {

constexpr uint32_t kLetters = 5;                              // A, C, G, T, N in the order of the tie rule
constexpr uint32_t kN = 4;
constexpr uint32_t kScoreBase = 33;                           // Phred+33
constexpr uint32_t kMaxQ = 93;                                // '~'
constexpr uint32_t kMax32 = 1u << 20;                         // members whose weights a Sum32 state holds, see (d)
constexpr uint32_t kChunk = 4;                                // columns a lane and load

// The tiers: a cluster of up to small members is a lane group's, of up to block a workgroup's, a larger one many workgroups'.
struct Tiers { uint32_t small, block, share; };               // share: members a workgroup of the last tier takes at most
constexpr Tiers kTiers{64u, kMax32 - 1u, 4096u};
constexpr Tiers kSmallTiers{8u, 64u, 16u};                    // FQD_CONSENSUS_SMALL_TIERS
static_assert(kTiers.block < kMax32 && kTiers.share <= kMax32 && kSmallTiers.block < kMax32, "(d): a workgroup's members fit Sum32");

template <class Sum>
struct State { Sum s[kLetters]; uint32_t mask; };
using State32 = State<uint32_t>;
using State64 = State<uint64_t>;

FQD_SEQ_HD uint32_t letter_of(uint8_t b) { return b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : kN; }
FQD_SEQ_HD uint8_t byte_of(uint32_t letter) { return letter == 0u ? 'A' : letter == 1u ? 'C' : letter == 2u ? 'G' : letter == 3u ? 'T' : 'N'; }
FQD_SEQ_HD uint32_t weight_of(uint32_t letter, uint8_t q) { return letter == kN || q < kScoreBase ? 0u : uint32_t(q) - kScoreBase; }

template <class Sum>
FQD_SEQ_HD void clear(State<Sum>& st)
{
    for (uint32_t x = 0; x < kLetters; ++x) st.s[x] = 0;
    st.mask = 0;
}

// One member's base and quality byte into a state.  (Every letter is tried so that s[] is never indexed by a value a
// register holds: the five sums stay in registers on the device.)
template <class Sum>
FQD_SEQ_HD void add(State<Sum>& st, uint8_t base, uint8_t q)
{
    const uint32_t l = letter_of(base), w = weight_of(l, q);
    for (uint32_t x = 0; x < kLetters; ++x) st.s[x] += x == l ? Sum(w) : Sum(0);
    st.mask |= 1u << l;
}

template <class Sum, class Other>
FQD_SEQ_HD void combine(State<Sum>& st, const State<Other>& o)
{
    for (uint32_t x = 0; x < kLetters; ++x) st.s[x] += Sum(o.s[x]);
    st.mask |= o.mask;
}

struct Verdict { uint32_t letter; uint8_t quality; bool changed; };   // changed: the winner is not the written member's letter

// What a column's state and the written member's own base byte make of it.  A state without a present letter (no member: the
// device never asks) gives the own letter and '!'.
template <class Sum>
FQD_SEQ_HD Verdict decide(const State<Sum>& st, uint8_t own_base)
{
    const uint32_t own = letter_of(own_base);
    uint32_t win = kLetters;
    Sum best = 0, total = 0;                                  // (the winner's sum as a value: s[] is never indexed by a register)
    for (uint32_t x = 0; x < kLetters; ++x) {
        total += st.s[x];
        if (!(st.mask >> x & 1u)) continue;
        if (win == kLetters || st.s[x] > best || (st.s[x] == best && x == own)) { win = x; best = st.s[x]; }   // (an earlier letter keeps a tie unless x is the own one)
    }
    if (win == kLetters) return Verdict{own, uint8_t(kScoreBase), false};
    int64_t q = int64_t(best) - int64_t(total - best);
    q = q < 0 ? 0 : q > int64_t(kMaxQ) ? int64_t(kMaxQ) : q;
    return Verdict{win, uint8_t(kScoreBase + uint32_t(q)), win != own};
}

// Whether record geometry allows the vote: the quality line, seq_len bytes at start + size - 1 - seq_len, lies behind the
// sequence line (and the byte that ends it) inside the record.
FQD_SEQ_HD bool lines_fit(uint64_t start, uint32_t size, uint64_t seq_off, uint32_t seq_len)
{
    if (uint64_t(size) < uint64_t(seq_len) + 1u || seq_off < start) return false;
    const uint64_t q_off = start + size - 1u - seq_len;
    if (seq_off > q_off) return false;
    return seq_len == 0u || q_off - seq_off > seq_len;        // (a difference: seq_off + seq_len may not fit 64 bits)
}

FQD_SEQ_HD uint64_t quality_at(uint64_t start, uint32_t size, uint32_t seq_len) { return start + size - 1u - seq_len; }

} // namespace fqdconsensus
