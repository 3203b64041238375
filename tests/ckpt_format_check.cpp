// ckpt_format_check.cpp -- the phi^4 ensemble checkpoint's format check (stochquant_amd/csrc/
// sq_phi4_ens_ckpt_format.cpp) as a stand-alone host program, built by tests/test_phi4_ens_checkpoint_format.py with
// the address and undefined-behaviour sanitizers: no HIP, nothing loaded into Python.
//
//   ckpt_format_check --sets MANIFEST      one line per set, "<json>\t<state>\t<field>": the three files read and
//                                          checked as a load checks them before it looks at its handle; prints
//                                          "accepted" or "refused: <why>" per line
//   ckpt_format_check --prefixes JSON      the metadata file cut at every length below its own: prints
//                                          "prefixes <n> refused <k>"
//   ckpt_format_check --path PATH          sq::ckpt::read_checkpoint(PATH, verify) itself
// Exit status 0 unless an argument is wrong; a sanitizer report ends the program with its own status.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../stochquant_amd/csrc/sq_phi4_ens_ckpt_format.h"

using namespace sq::ckpt;

static bool check_set(const std::string &json, const std::string &state, const std::string &field, std::string *why) {
    std::vector<unsigned char> j, s, f;
    Meta m;
    if (!read_file(json, &j, why) || !parse_meta(std::string(j.begin(), j.end()), &m, why)) return false;
    if (!read_file(state, &s, why) || !check_state_file(m, s, why)) return false;
    return read_file(field, &f, why) && check_field_file(m, f, why);
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const std::string mode = argv[1];
    std::string why;
    if (mode == "--sets") {
        std::ifstream in(argv[2]);
        if (!in) return 2;
        std::string line;
        while (std::getline(in, line)) {
            const size_t a = line.find('\t'), b = line.find('\t', a + 1);
            if (a == std::string::npos || b == std::string::npos) return 2;
            why.clear();
            if (check_set(line.substr(0, a), line.substr(a + 1, b - a - 1), line.substr(b + 1), &why))
                printf("accepted\n");
            else
                printf("refused: %s\n", why.c_str());
        }
        return 0;
    }
    if (mode == "--prefixes") {
        std::vector<unsigned char> j;
        if (!read_file(argv[2], &j, &why)) return 2;
        const std::string text(j.begin(), j.end());
        size_t refused = 0;
        for (size_t n = 0; n < text.size(); ++n) {
            Meta m;
            if (!parse_meta(text.substr(0, n), &m, &why)) ++refused;
        }
        printf("prefixes %zu refused %zu\n", text.size(), refused);
        return 0;
    }
    if (mode == "--path") {
        Meta m;
        if (read_checkpoint(argv[2], true, &m, nullptr, nullptr, &why))
            printf("accepted\n");
        else
            printf("refused: %s\n", why.c_str());
        return 0;
    }
    return 2;
}
