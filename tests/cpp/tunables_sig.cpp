// Every switch the environment can set must change tunables_signature(): tunables_refresh() compares signatures only, so a
// switch the signature leaves out is never read again once a process has read the switches (CPU only, g++).
// argv[1..]: the names tunables_from_environment() reads (tests/test_tunables_cpu.py takes them from the header's text).
#include "tunables.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>

int main(int argc, char **argv)
{
    for (int i = 1; i < argc; ++i) unsetenv(argv[i]);
    const std::string base = rsreg::tunables_signature();
    int missing = 0;
    for (int i = 1; i < argc; ++i) {
        setenv(argv[i], "1", 1);
        const std::string one = rsreg::tunables_signature();
        setenv(argv[i], "0", 1);
        const std::string zero = rsreg::tunables_signature();
        unsetenv(argv[i]);
        if (one == base || zero == one || rsreg::tunables_signature() != base) {
            std::printf("not in the signature: %s\n", argv[i]);
            ++missing;
        }
    }
    if (!missing) std::printf("signature ok: %d names\n", argc - 1);
    return missing ? 1 : 0;
}
