// The hand-written map of the host programs (host_abi.cpp, host_handle.cpp).  Include after smx_host.h.
#pragma once
#include <vector>

// A hand-written map — two roads, three lanes (0 and 1 on road 0 lead on to lane 2 on road 1), four lanepoints a
// lane, grids of 2 x 2 cells
struct Map {
  std::vector<int32_t> lane_road{0, 0, 1}, lane_index{0, 1, 0}, lane_shape_off{0, 2, 4, 6}, lane_out_off{0, 1, 2, 2}, lane_out_idx{2, 2};
  std::vector<int32_t> lane_in_off{0, 0, 0, 2}, lane_in_idx{0, 1}, road_par_off{0, 1, 1}, road_par_idx{1}, road_lane_off{0, 2, 3};
  std::vector<int32_t> road_lanes{0, 1, 2}, road_out_road{1, -1}, lpg_off{0, 3, 6, 9, 12}, sg_off{0, 1, 2, 3, 3};
  std::vector<double> lane_width{3.0, 3.5, 3.2}, lane_speed{10, 10, 10}, lane_length{30, 30, 30}, shape_x{0, 30, 0, 30, 30, 60}, shape_y{0, 0, 3, 3, 1, 1};
  std::vector<uint8_t> lane_in_junction{0, 0, 0}, road_is_junction{0, 0};
  std::vector<smx_shape_rec> shape_rec = std::vector<smx_shape_rec>(6);
  std::vector<smx_lp_rec> lp = std::vector<smx_lp_rec>(12);
  std::vector<smx_succ_rec> succ;
  std::vector<smx_pt_rec> lpg_pts = std::vector<smx_pt_rec>(12);
  std::vector<smx_seg_rec> sg = std::vector<smx_seg_rec>(3);
  smx_map_tables t{};
  Map() {
    for (int i = 0; i < 12; ++i) {
      smx_lp_rec& r = lp[i];
      r = smx_lp_rec{};
      r.lane = i / 4;
      const int next = i % 4 < 3 ? i + 1 : i < 8 ? 8 : -1;
      r.next0 = r.knot_next = next;
      r.n_next = next >= 0;
      r.next_off = (int32_t)succ.size();
      if (next >= 0) succ.push_back(smx_succ_rec{next, next / 4, next, 1});
      lpg_pts[i] = smx_pt_rec{(double)i, 0.0, i, i / 4};
    }
    for (int i = 0; i < 3; ++i) sg[i] = smx_seg_rec{0, 0, 1, 1, 1.6, 30, 0, i, 2 * i};
    t.n_lanes = 3, t.n_roads = 2, t.n_lanepoints = 12, t.n_shape_pts = 6, t.n_succ = (int32_t)succ.size();
    t.lane_road = lane_road.data(), t.lane_index = lane_index.data(), t.lane_width = lane_width.data(), t.lane_speed = lane_speed.data();
    t.lane_length = lane_length.data(), t.lane_in_junction = lane_in_junction.data(), t.lane_shape_off = lane_shape_off.data();
    t.shape_x = shape_x.data(), t.shape_y = shape_y.data(), t.shape_rec = shape_rec.data(), t.lane_out_off = lane_out_off.data();
    t.lane_out_idx = lane_out_idx.data(), t.road_lane_off = road_lane_off.data(), t.road_lanes = road_lanes.data();
    t.road_is_junction = road_is_junction.data(), t.road_out_road = road_out_road.data(), t.lp_rec = lp.data(), t.succ_rec = succ.data();
    t.lpg_cell = t.sg_cell = 32.0, t.lpg_nx = t.lpg_ny = t.sg_nx = t.sg_ny = 2;
    t.lpg_off = lpg_off.data(), t.lpg_pts = lpg_pts.data(), t.sg_off = sg_off.data(), t.sg_rec = sg.data(), t.default_lane_width = 3.2;
    t.lane_in_off = lane_in_off.data(), t.lane_in_idx = lane_in_idx.data(), t.road_par_off = road_par_off.data(), t.road_par_idx = road_par_idx.data();
  }
};
