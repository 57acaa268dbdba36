# The library's sources and headers, once, for every build of them: this directory's
# Makefile (all, stamps, diag, asm) and the host-sanitizer build of the C-ABI
# (tests/asan/Makefile). File names are relative to this directory.
GF_SRCS := flock_kernels.hip flock_rollout.hip flock_policy_rollout.hip flock_reset.hip flock_dt_noise.hip capi.hip flock_comm.hip coverage_kernels.hip coverage_expert.hip \
           coverage_maps.hip coverage_arl.hip coverage_hidden.hip coverage_reset.hip coverage_rollout.hip cov_capi.hip cov_maps_capi.hip cov_step_capi.hip \
           graph_utils.hip shepherd.hip shepherd_rollout.hip
GF_HDRS := flock_internal.h flock_dynamics.h flock_rollout_shared.h coverage_internal.h coverage_hidden.h coverage_step.h coverage_reset_draw.h mt19937.h done_flag.h device_alloc.h capi_common.h flock_handle.h \
           cov_handle.h net_delta.h shepherd_internal.h \
           ../../include/gymflock.h
