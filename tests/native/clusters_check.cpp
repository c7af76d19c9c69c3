// clusters_check.cpp — the words of the `--fast` units' cluster walk (fastq-dupaway_amd/csrc/fqd_clusters_core.hpp) on the CPU,
// the way the device and the launchers use them.  tests/test_clusters_core.py builds this with the sanitizers.
//   clusters_check entry < lines "k0 s"          > per line "entry place members"
//   clusters_check bad   < lines "record reason" > per line "word record reason"
//   clusters_check none                          > kNoBad
//   clusters_check room  < lines "n bound"       > list_room(n, bound) per line
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../fastq-dupaway_amd/csrc/fqd_clusters_core.hpp"

using namespace fqdclusters;

static int entries()
{
    unsigned long long k0, s;
    while (std::scanf("%llu %llu", &k0, &s) == 2) {
        const unsigned long long e = entry(uint32_t(k0), uint32_t(s));
        std::printf("%llu %" PRIu64 " %u\n", e, entry_place(e), entry_members(e));
    }
    return 0;
}

static int bad()
{
    unsigned long long record;
    unsigned reason;
    while (std::scanf("%llu %u", &record, &reason) == 2) {
        const unsigned long long w = bad_word(record, reason);
        uint64_t got_record = 0;
        uint32_t got_reason = 0;
        bad_parts(w, &got_record, &got_reason);
        std::printf("%llu %" PRIu64 " %u\n", w, got_record, got_reason);
    }
    return 0;
}

static int none()
{
    std::printf("%llu\n", kNoBad);
    return 0;
}

static int room()
{
    unsigned long long n, bound;
    while (std::scanf("%llu %llu", &n, &bound) == 2) std::printf("%" PRIu64 "\n", list_room(n, bound));
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && std::strcmp(argv[1], "entry") == 0) return entries();
    if (argc == 2 && std::strcmp(argv[1], "bad") == 0) return bad();
    if (argc == 2 && std::strcmp(argv[1], "none") == 0) return none();
    if (argc == 2 && std::strcmp(argv[1], "room") == 0) return room();
    return 2;
}
