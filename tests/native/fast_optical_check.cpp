// CPU harness for FastModes::optical (host/fast_modes.cpp; tests/test_fast_optical_cli.py builds it with -Werror and the
// sanitizers): reads the switches from the environment and prints what the run asks of them, a line each —
// "optical D", "linked 0|1", "any 0|1", "names ...", "note ...", and "check ..." for FastModes::check with the command line
// given as arguments (unordered 0|1, devices N).  A refusal or a bad value prints "error ..." and "refusal ..." instead.
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
    try {
        const FastModes m = FastModes::from_env();
        std::printf("optical %u\nlinked %d\nany %d\nnames %s\nnote %s\n", m.optical, int(m.linked()), int(m.any()), m.names().c_str(), m.out_of_memory_note().c_str());
        std::printf("reason %s\n", optical_reason(1).c_str());
        m.check(unordered, devices, Format::Fastq);
        std::printf("check passed\n");
    } catch (const FastModeRefusal& r) {
        std::printf("refusal %s\n", r.what());
    } catch (const std::exception& x) {
        std::printf("error %s\n", x.what());
    }
    return 0;
}
