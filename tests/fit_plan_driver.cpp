// Stand-alone driver of csrc/fit_plan.hpp for tests/test_fit_plan.py (plain g++, its own main; no HIP, no GPU):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I turbo_amd/csrc tests/fit_plan_driver.cpp -o <tmp>/fit_plan
//
//   fit_plan sizes          one line per Np = 256 .. 12288 in steps of 256 (N = Np): "Np OB nblk tail bginv"
//   fit_plan panels N Np    one line per outer block: "O tiles0 mode"  (mode: fused | pivot_beside | plain<variant>)
// The TGP_* switches come from the environment, as in the library.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fit_plan.hpp"

int main(int argc, char **argv) {
    const tgp::Tuning tu;
    if (argc == 2 && !strcmp(argv[1], "sizes")) {
        for (int Np = 256; Np <= 12288; Np += 256) {
            const tgp::FitPlan p = tgp::plan_fit(Np, Np, tu);
            printf("%d %d %d %d %d\n", Np, p.OB, p.nblk, p.tail(), p.bginv ? 1 : 0);
        }
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "panels")) {
        const tgp::FitPlan p = tgp::plan_fit(atoi(argv[2]), atoi(argv[3]), tu);
        for (int O = 0; O < p.Nr; O += p.OB) {
            const tgp::PanelMode m = p.panel_mode(O);
            if (m == tgp::PANEL_PLAIN) printf("%d %d plain%d\n", O, p.first_update_tiles(O), p.panel_var);
            else printf("%d %d %s\n", O, p.first_update_tiles(O), m == tgp::PANEL_FUSED ? "fused" : "pivot_beside");
        }
        return 0;
    }
    fprintf(stderr, "usage: fit_plan sizes | fit_plan panels N Np\n");
    return 2;
}
