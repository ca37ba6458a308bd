// Host-only sanitizer build (make asan): the parsers of untrusted files (csrc/cache.cpp, csrc/tree_io.cpp) compiled with
// -fsanitize=address,undefined and linked against these stand-ins for the entries that need a GPU.  Nothing here is product code.
#include <hip/hip_runtime_api.h>

#include "../../include/dvpari.h"
#include "../../include/dvpari_internal.h"
#include "../../dv-pari_amd/csrc/host_api.h"  // g_last_error_index is declared there; the other stand-ins are C ABI entries (dvpari.h)

namespace dvp {
thread_local int64_t g_last_error_index = -1;  // capi.cpp's in the product
}

extern "C" {
int64_t dvp_last_error_index(void) { return dvp::g_last_error_index; }
int dvp_prover_create(uint32_t, uint32_t, uint32_t, dvp_prover**) { return DVP_EHIP; }
void dvp_prover_destroy(dvp_prover*) {}
int dvp_prover_set_coeffs(dvp_prover*, const uint64_t*, uint32_t) { return DVP_EHIP; }
int dvp_prover_set_matrix(dvp_prover*, int, uint32_t, const uint32_t*, const uint32_t*, const uint32_t*) { return DVP_EHIP; }
int dvp_prover_set_srs_encoded(dvp_prover*, int, const uint8_t*, size_t) { return DVP_EHIP; }
int dvp_prover_srs_hash(dvp_prover*, uint8_t*) { return DVP_EHIP; }
int dvp_prover_circuit_hash(dvp_prover*, uint8_t*) { return DVP_EHIP; }
int dvp_prover_set_transcript_binding(dvp_prover*, const uint8_t*, const uint8_t*) { return DVP_EHIP; }
int dvp_prove(dvp_prover*, const uint64_t*, uint32_t, const uint64_t*, uint32_t, uint8_t*) { return DVP_EHIP; }
int dvp_prove_be32(dvp_prover*, const uint8_t*, size_t, uint8_t*) { return DVP_EHIP; }
int dvp_prove_ark(dvp_prover*, const uint64_t*, uint32_t, const uint64_t*, uint32_t, uint8_t*) { return DVP_EHIP; }
int dvp_prover_check_witness_be32(dvp_prover*, const uint8_t*, size_t, dvp_unsat_row*, size_t, dvp_suspect_wire*, size_t, dvp_witness_report*) { return DVP_EHIP; }
int dvp_prover_srs_slot_add(dvp_prover*, uint32_t*) { return DVP_EHIP; }
int dvp_prover_srs_slot_select(dvp_prover*, uint32_t) { return DVP_EHIP; }
uint32_t dvp_prover_srs_slot_active(const dvp_prover*) { return 0; }
int dvp_prover_srs_slot_drop(dvp_prover*, uint32_t) { return DVP_EHIP; }
size_t dvp_prover_msm_size(const dvp_prover*, int) { return 0; }
int dvp_prove_multi(dvp_prover*, const uint32_t*, uint32_t, const uint64_t*, uint32_t, const uint64_t*, uint32_t, uint8_t*, int32_t*) { return DVP_EHIP; }
int dvp_prove_multi_be32(dvp_prover*, const uint32_t*, uint32_t, const uint8_t*, size_t, uint8_t*, int32_t*) { return DVP_EHIP; }
int dvp_prove_multi_ark(dvp_prover*, const uint32_t*, uint32_t, const uint64_t*, uint32_t, const uint64_t*, uint32_t, uint8_t*, int32_t*) { return DVP_EHIP; }
int dvp_tune_get(const char*, long long* v) { if (v) *v = 1; return DVP_OK; }
hipError_t hipGetDevice(int* d) { if (d) *d = 0; return hipSuccess; }
hipError_t hipMemGetInfo(size_t* f, size_t* t) { if (f) *f = 0; if (t) *t = 0; return hipSuccess; }
}
