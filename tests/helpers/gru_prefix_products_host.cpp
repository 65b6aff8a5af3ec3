// g++ build of csrc/nlc_gru_prefix.h for tests/test_gru_prefix_products_host.py: where a table entry's hidden-side products sit.
#include "../../neurallaplacecontrol_amd/csrc/nlc_gru_prefix.h"

using namespace nlc::prefix;

extern "C" {
int nlc_gpp_starts_tile(int len, int B) { return starts_tile(len, B) ? 1 : 0; }
int nlc_gpp_build_steps(int B) { return build_steps(B); }
long nlc_gpp_products_doubles(int g) { return (long)products_doubles(g); }
long nlc_gpp_products_entry_offset(int entry, int g) { return (long)products_entry_offset(entry, g); }
int nlc_gpp_products_index(int layer, int j, int set, int q, int r, int g) { return products_index(layer, j, set, q, r, g); }
}
