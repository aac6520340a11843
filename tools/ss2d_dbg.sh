#!/bin/bash
# stage removal in the chunked SS2D passes (results wrong on purpose): per-variant libraries, timed with tools/ss2d_bench.py
# (XP_SS2D_DBG is read in csrc/ss2d_core.h; the kernels that use it are in csrc/ss2d_chunked.hip and, through step_vals, csrc/ss2d_seq.hip)
for d in ${SS2D_DBG_SET:-0 1 2 3}; do
  touch xpoint_amd/csrc/ss2d_chunked.hip xpoint_amd/csrc/ss2d_seq.hip
  XP_EXTRA_HIPCC_FLAGS="-DXP_SS2D_DBG=$d" python -m xpoint_amd.build > /dev/null 2>&1 || echo build failed
  cp xpoint_amd/libxpoint_hip.so xpoint_amd/libxp_ss2d_dbg$d.so
done
touch xpoint_amd/csrc/ss2d_chunked.hip xpoint_amd/csrc/ss2d_seq.hip; python -m xpoint_amd.build > /dev/null 2>&1
