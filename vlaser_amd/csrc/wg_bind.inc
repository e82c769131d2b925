// A body file (*.inc) as a stand-alone __global__ kernel: its workgroup indices are the launch's own.  Include in front of the body, wg_unbind.inc behind it.  (A __device__
// body that also runs as the guest of another kernel's launch defines the same five names itself, from its arguments, and shares wg_unbind.inc.)
#define VL_WG_X blockIdx.x
#define VL_WG_Y blockIdx.y
#define VL_WG_Z blockIdx.z
#define VL_GRID_X gridDim.x
#define VL_GRID_Y gridDim.y
