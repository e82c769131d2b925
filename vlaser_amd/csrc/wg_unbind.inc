// Behind an included body file: drops the workgroup-index names (wg_bind.inc, or the five defines of a __device__ body).
#undef VL_WG_X
#undef VL_WG_Y
#undef VL_WG_Z
#undef VL_GRID_X
#undef VL_GRID_Y
