// CPU harness for csrc/fqd_centroid_core.hpp (tests/test_centroid_core.py builds it with -Werror and the sanitizers): the
// header's host compile, driven the way the device tiers drive it, one lane after the other.
//   runs     every run of 1 .. 6 members: every way its members share labels (restricted growth strings in lexicographic
//            order, label value (7 * id + 3) % 11) x every weight of {1, 2, 2^31 - 1} a member (member i's is digit i of a
//            base-3 counter).  The abundances come from the table in LDS's helpers AND from the table in scratch's (head
//            place 2^31 - 2), which must agree; the centroid from better(); the masked scores of the fixed scores kScore
//            against the centroid's label, and the member a second pick takes.  A line a run:
//            "<abundances,> <centroid> <masked,> <best>".
//   tables   stdin: "<head place> <label> <weight>" a member of ONE run; both tables as above, a line a member: its abundance.
//   slots    stdin: "<label> <members>": block_slots, block_slot; "<head place> <label> <members>": scratch_slots, scratch_slot
//            and the packed key, as hex.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../fastq-dupaway_amd/csrc/fqd_centroid_core.hpp"

using namespace fqdcentroid;

static void fail(const char* what) { std::printf("FAILED %s\n", what); std::exit(1); }

// A workgroup's tier: the table in LDS, a member after the other.
static std::vector<uint64_t> by_block_table(const std::vector<uint32_t>& label, const std::vector<uint32_t>& weight)
{
    const uint32_t s = uint32_t(label.size()), slots = block_slots(s);
    if (slots < 2 * s && s <= kBlockLimit) fail("block_slots below twice the members");
    std::vector<uint32_t> keys(slots, kNoLabel), at(s);
    std::vector<uint64_t> sums(slots, 0), out(s);
    for (uint32_t v = 0; v < s; ++v) {
        uint32_t slot = block_slot(label[v], slots), tries = 0;
        if (slot >= slots) fail("block_slot outside the table");
        while (keys[slot] != kNoLabel && keys[slot] != label[v]) { slot = uint32_t(next_slot(slot, slots)); if (++tries > slots) fail("no empty slot in LDS"); }
        keys[slot] = label[v]; sums[slot] += weight[v]; at[v] = slot;
    }
    for (uint32_t v = 0; v < s; ++v) out[v] = sums[at[v]];
    return out;
}

// The large tier: the table in scratch, first every add, then every look-up.
static std::vector<uint64_t> by_scratch_table(uint32_t head_place, const std::vector<uint32_t>& label, const std::vector<uint32_t>& weight)
{
    const uint64_t s = label.size(), slots = scratch_slots(s);
    std::vector<uint64_t> keys(slots, kNoKey), sums(slots, 0), out(s);
    for (uint64_t v = 0; v < s; ++v) {
        const uint64_t key = pack_key(head_place, label[v]);
        if (key == kNoKey) fail("a key that is the empty slot's");
        uint64_t slot = scratch_slot(key, slots), tries = 0;
        if (slot >= slots) fail("scratch_slot outside the table");
        while (keys[slot] != kNoKey && keys[slot] != key) { slot = next_slot(slot, slots); if (++tries > slots) fail("no empty slot in scratch"); }
        keys[slot] = key; sums[slot] += weight[v];
    }
    for (uint64_t v = 0; v < s; ++v) {
        const uint64_t key = pack_key(head_place, label[v]);
        uint64_t slot = scratch_slot(key, slots);
        while (keys[slot] != key) slot = next_slot(slot, slots);
        out[v] = sums[slot];
    }
    return out;
}

static const uint32_t kScore[6] = {5u, 0xFFFFFFFFu, 0xFFFFFFFEu, 0u, 7u, 5u};
static const uint32_t kWeights[3] = {1u, 2u, 0x7FFFFFFFu};

static void one_run(const std::vector<uint32_t>& id, uint32_t code)
{
    const uint32_t s = uint32_t(id.size());
    std::vector<uint32_t> label(s), weight(s);
    for (uint32_t i = 0; i < s; ++i) { label[i] = (7u * id[i] + 3u) % 11u; weight[i] = kWeights[code % 3u]; code /= 3u; }
    const std::vector<uint64_t> a = by_block_table(label, weight), b = by_scratch_table(0x7FFFFFFEu, label, weight);
    if (a != b) fail("the two tables disagree");
    uint32_t c = 0;
    for (uint32_t i = 1; i < s; ++i) if (better(saturate(a[i]), i, saturate(a[c]), c)) c = i;
    // the order behind the exchange: the centroid in front, the former first member at its place
    std::vector<uint32_t> order(s);
    for (uint32_t i = 0; i < s; ++i) order[i] = i;
    order[0] = c; order[c] = 0;
    std::vector<uint32_t> masked(s);
    for (uint32_t i = 0; i < s; ++i) masked[i] = masked_score(kScore[i], label[i] == label[c]);
    uint32_t best = 0;                                         // a place of `order`
    for (uint32_t k = 1; k < s; ++k) if (better(masked[order[k]], k, masked[order[best]], best)) best = k;
    for (uint32_t i = 0; i < s; ++i) std::printf("%s%" PRIu32, i ? "," : "", saturate(a[i]));
    std::printf(" %" PRIu32 " ", c);
    for (uint32_t i = 0; i < s; ++i) std::printf("%s%" PRIu32, i ? "," : "", masked[i]);
    std::printf(" %" PRIu32 "\n", order[best]);
}

// used: the ids in front are 0 .. used - 1; the next member takes one of them or the next free one.
static void grow(std::vector<uint32_t>& id, uint32_t s, uint32_t used)
{
    if (id.size() == s) {
        uint32_t codes = 1;
        for (uint32_t i = 0; i < s; ++i) codes *= 3u;
        for (uint32_t code = 0; code < codes; ++code) one_run(id, code);
        return;
    }
    for (uint32_t v = 0; v <= used; ++v) {
        id.push_back(v);
        grow(id, s, v == used ? used + 1u : used);
        id.pop_back();
    }
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    if (!std::strcmp(argv[1], "runs")) {
        for (uint32_t s = 1; s <= 6; ++s) { std::vector<uint32_t> id; grow(id, s, 0); }
        return 0;
    }
    if (!std::strcmp(argv[1], "tables")) {
        std::vector<uint32_t> label, weight;
        uint32_t head_place = 0, l, w;
        while (std::scanf("%" SCNu32 " %" SCNu32 " %" SCNu32, &head_place, &l, &w) == 3) { label.push_back(l); weight.push_back(w); }
        const std::vector<uint64_t> b = by_scratch_table(head_place, label, weight);
        if (label.size() <= kBlockLimit && by_block_table(label, weight) != b) fail("the two tables disagree");
        for (uint64_t v : b) std::printf("%" PRIu32 "\n", saturate(v));
        return 0;
    }
    if (!std::strcmp(argv[1], "slots")) {
        char line[128];
        while (std::fgets(line, sizeof line, stdin)) {
            uint32_t x, y, z;
            const int got = std::sscanf(line, "%" SCNu32 " %" SCNu32 " %" SCNu32, &x, &y, &z);
            if (got == 2) std::printf("%" PRIu32 " %" PRIu32 " %" PRIu32 "\n", block_slots(y), block_slot(x, block_slots(y)), tier_of(y));
            else if (got == 3) std::printf("%" PRIu64 " %" PRIu64 " %" PRIx64 "\n", scratch_slots(z), scratch_slot(pack_key(x, y), scratch_slots(z)), pack_key(x, y));
        }
        return 0;
    }
    return 2;
}
