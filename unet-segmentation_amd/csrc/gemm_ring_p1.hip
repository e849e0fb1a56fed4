// k_gemm_ring tiles 94-96 (see gemm_ring.hip: the tiles compile in three units)
#define GEMM_RING_PART 1
#include "gemm_ring.hip"
