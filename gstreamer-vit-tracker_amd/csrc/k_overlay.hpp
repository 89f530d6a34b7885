// k_overlay.hpp — launchers of the command-list overlays (k_overlay.hip).
#pragma once
#include "vt_common.hpp"
#include "../../include/vittrack_hip.h"

hipError_t launch_overlay(uint8_t* yplane, int width, int height, int stride, const vt_draw_cmd* d_cmds,
                          int n, hipStream_t st);

hipError_t launch_overlay_rgb(uint8_t* rgb, int width, int height, int stride, const vt_draw_cmd* d_cmds,
                              int n, hipStream_t st);
