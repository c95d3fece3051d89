"""learnraytracing_amd — MI355X-native drop-in for the per-pixel path tracer of
Sefaice/LearnRayTracing's src/cpu renderer (TraceRowJob -> Trace -> HitWorld/HitSphere
-> Scatter -> progressive backbuffer), as a hand-written HIP megakernel for gfx950
behind the C-ABI of include/lrt.h.

Python is the host-side mirror of the reference API; the compute path is
liblrt_hip.so only (no CPU fallback).
"""
from ._lib import LrtError, lib  # noqa: F401
from .renderer import (DrawTest, InitializeDevices, InitializeTest, Job, ShutdownTest,  # noqa: F401
                       TemporalAccumulator, ToneMapper, default_camera, denoise_desc, denoise_host, denoise_tensor, device_count, make_camera,
                       pinned_backbuffer, get_scene, render_device, render_host, render_host_features,
                       render_tensor, render_tensor_features, render_tensor_to_frame, set_scene, shard_rows,
                       svgf_desc, svgf_filter_host, svgf_filter_tensor,
                       temporal_accumulate_host, temporal_accumulate_moving_host, temporal_accumulate_moving_tensor,
                       temporal_accumulate_tensor, temporal_desc,
                       temporal_accumulate_gbuffer_host, temporal_accumulate_gbuffer_tensor, temporal_gbuffer_desc,
                       tonemap_desc, tonemap_host, tonemap_tensor,
                       gbuffer_desc, gbuffer_host, gbuffer_tensor,
                       gbuffer_chain_desc, gbuffer_chain_host, gbuffer_chain_tensor,
                       gbuffer_chain_motion_desc, gbuffer_chain_motion_host, gbuffer_chain_motion_tensor,
                       upsample_desc, upsample_host, upsample_tensor,
                       TemporalUpsampler, jitter_camera, jitter_phases, temporal_upsample_desc,
                       temporal_upsample_host, temporal_upsample_tensor,
                       temporal_rectify_desc, temporal_rectify_host, temporal_rectify_tensor,
                       sample_budget_desc, sample_budget_host, sample_budget_tensor,
                       render_counts_host, render_counts_tensor,
                       firefly_desc, firefly_host, firefly_tensor,
                       firefly_restore_desc, firefly_restore_host, firefly_restore_tensor)
from .scene import default_scene, random_scene  # noqa: F401

__version__ = "0.4.0"
