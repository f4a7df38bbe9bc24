"""ctypes binding of libhobbyrt_pt.so (include/hobbyrt_pt.h), one module per pt_capi_*.cpp. There is no fallback: if the in-tree HIP
library is missing this package raises at import, and if no GPU is present hrpt_create fails."""
import ctypes as C  # noqa: F401

from ._lib import EXPORTS, LIB_PATH, HrptError, lib  # noqa: F401
from .atmosphere import (ATM_PASS_DENSITY, ATM_PASS_DIRECT_IRRADIANCE, ATM_PASS_INDIRECT, ATM_PASS_MULTIPLE, ATM_PASS_SINGLE,  # noqa: F401
                         ATM_PASS_TRANSMITTANCE, ATMOSPHERE_ORDERS, _atmosphere_cache_path, atmosphere_pass, precompute_atmosphere)
from .context import PathTracerContext, allgather  # noqa: F401
from .geometry import Animation, _aligned_copy, animation_desc, quantize_vertices_host, skin_arrays, skin_vertices_host  # noqa: F401
from .lighting import (deferred_rays_host, deferred_shade_host, indirect_compose_host, indirect_rays_host, indirect_resolve_host,  # noqa: F401
                       restir_initial_host, restir_shade_host, restir_spatial_host, restir_temporal_host)
from .post import (bloom_host, bloom_pack_probe, compose_host, demodulate_host, denoise_host, modulation_probe, noise_tile_from_png,  # noqa: F401
                   temporal_host, upscale_host)
from .probes import ProbeVolume, probe_points, probe_volume, probes_blend_host, probes_query_host, probes_rays_host  # noqa: F401
from .rcache import RadianceCache, rcache_desc, rcache_insert_host, rcache_query_host, rcache_resolve_host, rcache_table  # noqa: F401
from .selftest import host_build_bvh  # noqa: F401
