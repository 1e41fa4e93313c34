// jobplan_sanitize.cc -- every request of tests/golden/cli_table.json through plan_job and refuse_on_session (src/mgm_jobplan.h)
// in a program of its own, for a run under the host sanitizers (never loaded into Python, never near a device):
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I src tests/jobplan_sanitize.cc -o /tmp/jobplan_sanitize
//   python tests/test_jobplan.py --rows | /tmp/jobplan_sanitize
// stdin: per request the lines `T token` and `E name=value`, then a line with a dot.  Prints how many it planned and a checksum.
#include <iostream>
#include <map>

#include "mgm_jobplan.h"

int main()
{
    std::vector<std::string> tok;
    std::map<std::string, std::string> env;
    std::string line;
    size_t n = 0, sum = 0;
    while (std::getline(std::cin, line)) {
        if (line.rfind("T ", 0) == 0) tok.push_back(line.substr(2));
        else if (line.rfind("E ", 0) == 0) env[line.substr(2, line.find('=') - 2)] = line.substr(line.find('=') + 1);
        if (line != ".") continue;
        const mgm_cli::JobPlan p = mgm_cli::plan_job(tok, [&](const char *name) {
            const auto it = env.find(name);
            return it == env.end() ? nullptr : it->second.c_str();
        });
        sum += p.code + p.out_text.size() + p.err_text.size() + p.devices.size() + p.iterations;
        for (int multi = 0; multi < 2; multi++)
            for (int v_ny = 47; v_ny < 49; v_ny++) sum += mgm_cli::refuse_on_session(p, multi != 0, 48, v_ny).err_text.size();
        tok.clear();
        env.clear();
        n++;
    }
    printf("%zu requests planned, checksum %zu\n", n, sum);
    return n ? 0 : 1;
}
