// compile_callers_localmapping.cc -- compile-only check of the drop-in claim for LocalMapping::CreateNewMapPoints: the reference's call line
// in LocalMapping::Run (src/LocalMapping.cc:87-92, :105-109) against the LocalMapping stand-in of host/slam_types.h.  Nothing here runs.
// Built by `make lib/compile_callers_localmapping.o` with -Wall -Werror, asserted by tests/test_new_points_abi.py.
#include "slam_types.h"

using namespace std;

namespace ORB_SLAM3 {

struct LocalMappingRun : public LocalMapping {
    void MapPointCulling() {}
    void SearchInNeighbors() {}
    // LocalMapping::Run, :87-92 and :105-109
    void RunOnce()
    {
            // Check recent MapPoints
            MapPointCulling();

            // Triangulate new MapPoints
            CreateNewMapPoints();

            if(!CheckNewKeyFrames())
            {
                // Find more matches in neighbor keyframes and fuse point duplications
                SearchInNeighbors();
            }
    }
};

void local_mapping_run_once(LocalMappingRun &lm) { lm.RunOnce(); }

}  // namespace ORB_SLAM3
