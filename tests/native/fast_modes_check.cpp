// fast_modes_check.cpp — the FQD_FAST_* switches as one value (fastq-dupaway_amd/host/fast_modes.hpp) on their own: no GPU
// call, no HIP.  tests/test_fast_modes.py builds this with host/fast_modes.cpp and the sanitizers.
//   fast_modes_check < one case per line, tab-separated: "unordered devices fastq|fasta NAME=VALUE ..."
// Every FQD_FAST_* variable is unset, the named ones are set (setenv), then FastModes::from_env() and check() run
// (unordered "-": from_env() alone).
//   > "value <message>"    from_env threw something that is no FastModeRefusal
//   > "refusal <message>"  from_env or check threw FastModeRefusal
//   > "ok" and, tab-separated: keep_best clusters both_strands umi umi_mismatch size_out levels sort_by_size min_size
//     max_size size_in | size_filter() sized() linked() any() | names() | out_of_memory_note()
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../fastq-dupaway_amd/host/fast_modes.hpp"

using fqdhost::detail::FastModeRefusal;
using fqdhost::detail::FastModes;

static const char* const kVariables[] = {"FQD_FAST_KEEP", "FQD_FAST_CLUSTERS", "FQD_FAST_STRAND", "FQD_FAST_UMI", "FQD_FAST_UMI_MISMATCH", "FQD_FAST_SIZEOUT",
                                         "FQD_FAST_LEVELS", "FQD_FAST_SORT", "FQD_FAST_MINSIZE", "FQD_FAST_MAXSIZE", "FQD_FAST_SIZEIN"};

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::vector<std::string> field;
        std::stringstream in(line);
        for (std::string f; std::getline(in, f, '\t');) field.push_back(f);
        if (field.size() < 3) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
        for (const char* name : kVariables) unsetenv(name);
        for (size_t k = 3; k < field.size(); ++k) {
            const size_t eq = field[k].find('=');
            if (eq == std::string::npos) { std::fprintf(stderr, "bad setting: %s\n", field[k].c_str()); return 2; }
            setenv(field[k].substr(0, eq).c_str(), field[k].substr(eq + 1).c_str(), 1);
        }
        try {
            const FastModes m = FastModes::from_env();
            if (field[0] != "-") m.check(field[0] == "1", size_t(std::atoi(field[1].c_str())), field[2] == "fasta" ? fqdhost::Format::Fasta : fqdhost::Format::Fastq);
            std::cout << "ok\t" << m.keep_best << ' ' << m.clusters << ' ' << m.both_strands << ' ' << m.umi << ' ' << m.umi_mismatch << ' ' << m.size_out << ' ' << m.levels << ' '
                      << m.sort_by_size << ' ' << m.min_size << ' ' << m.max_size << ' ' << m.size_in << '\t' << m.size_filter() << ' ' << m.sized() << ' ' << m.linked() << ' '
                      << m.any() << '\t' << m.names() << '\t' << m.out_of_memory_note() << '\n';
        } catch (const FastModeRefusal& e) {
            std::cout << "refusal\t" << e.what() << '\n';
        } catch (const std::exception& e) {
            std::cout << "value\t" << e.what() << '\n';
        }
    }
    return 0;
}
