/* abi_check_ffjord_chain.c -- prints sizeof / offsetof of rnde_ffjord_chain_config (include/rnde.h) as a C compiler lays it out, in the
 * format of abi_check.c: one line per field, "<struct> <field> <offset> <size>", and "<struct> sizeof <bytes>".
 * tests/test_ffjord_chain_host.py compiles it with `gcc -I include` and compares the output with the ctypes mirror
 * (regneuralde.jl_amd/_lib.py) and with the field list of the Julia mirror (bindings/julia/RNDE.jl). */
#include <stddef.h>
#include <stdio.h>

#include "rnde.h"

#define F(S, f) printf(#S " " #f " %zu %zu\n", offsetof(S, f), sizeof(((S*)0)->f))

int main(void) {
    F(rnde_ffjord_chain_config, n_layers); F(rnde_ffjord_chain_config, dims); F(rnde_ffjord_chain_config, act);
    F(rnde_ffjord_chain_config, time_dep); F(rnde_ffjord_chain_config, regularize); F(rnde_ffjord_chain_config, max_batch);
    F(rnde_ffjord_chain_config, solver); F(rnde_ffjord_chain_config, reltol); F(rnde_ffjord_chain_config, abstol);
    F(rnde_ffjord_chain_config, cb_save_start); F(rnde_ffjord_chain_config, max_attempts); F(rnde_ffjord_chain_config, device);
    printf("rnde_ffjord_chain_config sizeof %zu\n", sizeof(rnde_ffjord_chain_config));
    return 0;
}
