// CPU harness for FastModes::centroid (host/fast_modes.cpp; tests/test_fast_centroid_modes.py builds it with -Werror and the
// sanitizers): reads the switches from the environment and prints what the run asks of them, a line each — "centroid 0|1",
// "merges 0|1", "linked 0|1", "any 0|1", "names ...", "note ...", and "check passed" for FastModes::check with the command line
// given as arguments (unordered 0|1, devices N, fasta 0|1).  A refusal or a bad value prints "refusal ..." or "error ..."
// instead of what would have followed.
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
        std::printf("centroid %d\nmerges %d\nlinked %d\nany %d\nnames %s\nnote %s\n", int(m.centroid), int(m.merges()), int(m.linked()), int(m.any()), m.names().c_str(),
                    m.out_of_memory_note().c_str());
        m.check(unordered, devices, fasta ? Format::Fasta : Format::Fastq);
        std::printf("check passed\n");
    } catch (const FastModeRefusal& r) {
        std::printf("refusal %s\n", r.what());
    } catch (const std::exception& x) {
        std::printf("error %s\n", x.what());
    }
    return 0;
}
