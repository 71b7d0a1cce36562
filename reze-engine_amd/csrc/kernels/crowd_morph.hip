// kernels/crowd_morph.hip — the MORPH = true half of the crowd kernels (inst_morphs: a crowd with sparse vertex morphs), in a translation
// unit of its own so that kernels/crowd.hip's build and its instantiations are what they were: kernels/crowd.hip again, which then
// instantiates rz_skin_instances_morph_kernel / rz_skin_instances_fk_morph_kernel and defines the two rz_launch_*_morph_half launchers
// for its rz_launch_skin_instances / rz_launch_skin_instances_fk.
#define RZ_CROWD_MORPH true
#include "crowd.hip"
