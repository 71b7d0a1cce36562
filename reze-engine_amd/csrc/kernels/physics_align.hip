// kernels/physics_align.hip — the ALIGN = true half of rz_physics_kernel's instantiations (rz_physics_aligned: a table with PMX type-2 bodies
// that are simulated), in a translation unit of its own so that it compiles beside the other half: kernels/physics.hip again, which then
// instantiates with ALIGN = true and defines rz_launch_physics_aligned_half for its rz_launch_physics.
#define RZ_PHYSICS_ALIGN true
#include "physics.hip"
