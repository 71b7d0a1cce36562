// kernels/crowd_morph.hip — the MORPH = true half of the crowd kernels (inst_morphs: a crowd with sparse vertex morphs), in a translation
// unit of its own so that kernels/crowd.hip's build and its instantiations are what they were: kernels/crowd.hip again, which then
// instantiates rz_skin_instances_morph_kernel / rz_skin_instances_fk_morph_kernel and exports its one launcher as rz_launch_crowd_morph
// (rz_launch_frame sends it the records with `morph` set).
#define RZ_CROWD_MORPH true
#include "crowd.hip"
