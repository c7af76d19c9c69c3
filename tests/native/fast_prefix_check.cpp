// CPU harness for FastModes::prefix and FastModes::longest (host/fast_modes.cpp; tests/test_fast_prefix_modes.py builds it with
// -Werror and the sanitizers): reads the switches from the environment and prints what the run asks of them, a line each —
// "prefix L", "longest 0|1", "centroid 0|1", "merges 0|1", "picks 0|1", "linked 0|1", "any 0|1", "names ...", "name ...",
// "note ...", and "check passed" for FastModes::check with the command line given as arguments (unordered 0|1, devices N,
// fasta 0|1).  A refusal or a bad value prints "refusal ..." or "error ..." instead of what would have followed.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../fastq-dupaway_amd/host/fast_modes.hpp"

using namespace fqdhost;
using namespace fqdhost::detail;

int main(int argc, char** argv)
{
    const bool unordered = argc > 1 && std::atoi(argv[1]) != 0;
    const size_t devices = argc > 2 ? size_t(std::atoi(argv[2])) : 1;
    const bool fasta = argc > 3 && std::atoi(argv[3]) != 0;
    try {
        const FastModes m = FastModes::from_env();
        std::printf("prefix %u\nlongest %d\ncentroid %d\nmerges %d\npicks %d\nlinked %d\nany %d\nnames %s\nname %s\nnote %s\n", m.prefix, int(m.longest), int(m.centroid),
                    int(m.merges()), int(m.picks_centroid()), int(m.linked()), int(m.any()), m.names().c_str(), m.prefix_name().c_str(), m.out_of_memory_note().c_str());
        m.check(unordered, devices, fasta ? Format::Fasta : Format::Fastq);
        std::printf("check passed\n");
    } catch (const FastModeRefusal& r) {
        std::printf("refusal %s\n", r.what());
    } catch (const std::exception& x) {
        std::printf("error %s\n", x.what());
    }
    return 0;
}
