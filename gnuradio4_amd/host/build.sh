#!/bin/bash
# builds the C++ host-layer test programs and the plugin (g++ -std=c++20); the four targets compile in parallel and only when stale
set -e
cd "$(dirname "$0")"
OUT=../../build/host
mkdir -p $OUT
HDRS="include/gr4/core.hpp include/gr4/converter_ops.hpp include/gr4/electrical_ops.hpp include/gr4/blocks.hpp include/gr4/merge.hpp include/gr4/hip.hpp include/gr4/plugin.hpp include/gr4/grc.hpp ../../include/gr4hip.h"
CXX="g++ -std=c++20 -Wall -Wextra -Iinclude"
LINK="-L.. -lgr4hip -Wl,-rpath,\$ORIGIN/../../gnuradio4_amd -Wl,-rpath,/opt/rocm/lib"
stale() { # target sources...
  local t=$1; shift
  [ ! -e "$t" ] && return 0
  for s in "$@" $HDRS ../libgr4hip.so; do [ "$s" -nt "$t" ] && return 0; done
  return 1
}
pids=()
# the CPU program links the library too: the filter-design and window functions behind BasicFilter / FFT are host code in libgr4hip.so
if stale $OUT/test_host_cpu tests/test_host_cpu.cpp; then $CXX -O2 tests/test_host_cpu.cpp -o $OUT/test_host_cpu $LINK & pids+=($!); fi
if stale $OUT/test_host_fanin tests/test_host_fanin.cpp; then $CXX -O2 tests/test_host_fanin.cpp -o $OUT/test_host_fanin $LINK & pids+=($!); fi
if stale $OUT/test_host_device tests/test_host_device.cpp; then $CXX -O2 tests/test_host_device.cpp -o $OUT/test_host_device $LINK & pids+=($!); fi
# the plugin (gr_plugin_make / gr_plugin_free) next to libgr4hip.so, and a loader test that links neither
# (the 246 converter block types are twelve translation units of the plugin, compiled side by side; the plugin is linked once everything is built)
PLUGIN_OBJS=""
if stale ../libgr4hip_blocks.so plugin/gr4hip_blocks.cpp plugin/gr4hip_converters.cpp; then
  PLUGIN_OBJS="$OUT/plugin_main.o"
  $CXX -O1 -fPIC -fvisibility=hidden -c plugin/gr4hip_blocks.cpp -o $OUT/plugin_main.o & pids+=($!)
  for k in 0 1 2 3 4 5 6 7 8 9 10 11; do
    PLUGIN_OBJS="$PLUGIN_OBJS $OUT/plugin_conv$k.o"
    $CXX -O1 -fPIC -fvisibility=hidden -DGR4HIP_CONVERTER_PART=$k -c plugin/gr4hip_converters.cpp -o $OUT/plugin_conv$k.o & pids+=($!)
  done
fi
if stale $OUT/bench_host_feed tests/bench_host_feed.cpp; then $CXX -O2 tests/bench_host_feed.cpp -o $OUT/bench_host_feed $LINK & pids+=($!); fi
if stale $OUT/bench_host_fanin tests/bench_host_fanin.cpp; then $CXX -O2 tests/bench_host_fanin.cpp -o $OUT/bench_host_fanin $LINK & pids+=($!); fi
if stale $OUT/dump_signal_generator tests/dump_signal_generator.cpp; then $CXX -O2 tests/dump_signal_generator.cpp -o $OUT/dump_signal_generator $LINK & pids+=($!); fi
if stale $OUT/test_host_plugin tests/test_host_plugin.cpp; then $CXX -O2 tests/test_host_plugin.cpp -o $OUT/test_host_plugin -ldl & pids+=($!); fi
if stale $OUT/test_host_freq_est tests/test_host_freq_est.cpp; then $CXX -O2 tests/test_host_freq_est.cpp -o $OUT/test_host_freq_est -ldl & pids+=($!); fi
if stale $OUT/test_host_iq_demod tests/test_host_iq_demod.cpp; then $CXX -O2 tests/test_host_iq_demod.cpp -o $OUT/test_host_iq_demod -ldl & pids+=($!); fi
if stale $OUT/test_host_power_metrics tests/test_host_power_metrics.cpp; then $CXX -O2 tests/test_host_power_metrics.cpp -o $OUT/test_host_power_metrics -ldl & pids+=($!); fi
if stale $OUT/test_host_schmitt_trigger tests/test_host_schmitt_trigger.cpp; then $CXX -O2 tests/test_host_schmitt_trigger.cpp -o $OUT/test_host_schmitt_trigger -ldl & pids+=($!); fi
if stale $OUT/test_host_svd_denoiser tests/test_host_svd_denoiser.cpp; then $CXX -O2 tests/test_host_svd_denoiser.cpp -o $OUT/test_host_svd_denoiser -ldl & pids+=($!); fi
if stale $OUT/test_host_signal_generator tests/test_host_signal_generator.cpp; then $CXX -O2 tests/test_host_signal_generator.cpp -o $OUT/test_host_signal_generator $LINK & pids+=($!); fi
if stale $OUT/test_host_converter tests/test_host_converter.cpp; then $CXX -O1 tests/test_host_converter.cpp -o $OUT/test_host_converter $LINK & pids+=($!); fi
if stale $OUT/test_host_electrical tests/test_host_electrical.cpp; then $CXX -O2 tests/test_host_electrical.cpp -o $OUT/test_host_electrical -ldl & pids+=($!); fi
if stale $OUT/test_host_savitzky_golay tests/test_host_savitzky_golay.cpp; then $CXX -O2 tests/test_host_savitzky_golay.cpp -o $OUT/test_host_savitzky_golay $LINK -ldl & pids+=($!); fi
if stale $OUT/test_host_complex_fir tests/test_host_complex_fir.cpp; then $CXX -O2 tests/test_host_complex_fir.cpp -o $OUT/test_host_complex_fir $LINK -ldl & pids+=($!); fi
if stale $OUT/test_host_pfb tests/test_host_pfb.cpp; then $CXX -O2 tests/test_host_pfb.cpp -o $OUT/test_host_pfb $LINK -ldl & pids+=($!); fi
if stale $OUT/test_host_stft tests/test_host_stft.cpp; then $CXX -O2 tests/test_host_stft.cpp -o $OUT/test_host_stft $LINK -ldl & pids+=($!); fi
if stale $OUT/test_host_ifft tests/test_host_ifft.cpp; then $CXX -O2 tests/test_host_ifft.cpp -o $OUT/test_host_ifft $LINK -ldl & pids+=($!); fi
if stale $OUT/test_host_rational_resampler tests/test_host_rational_resampler.cpp; then $CXX -O2 tests/test_host_rational_resampler.cpp -o $OUT/test_host_rational_resampler $LINK -ldl & pids+=($!); fi
if stale $OUT/test_host_spectrum_integrator tests/test_host_spectrum_integrator.cpp; then $CXX -O2 tests/test_host_spectrum_integrator.cpp -o $OUT/test_host_spectrum_integrator $LINK -ldl & pids+=($!); fi
if stale $OUT/test_host_cross_spectrum tests/test_host_cross_spectrum.cpp; then $CXX -O2 tests/test_host_cross_spectrum.cpp -o $OUT/test_host_cross_spectrum $LINK -ldl & pids+=($!); fi
if stale $OUT/test_host_beamformer tests/test_host_beamformer.cpp; then $CXX -O2 tests/test_host_beamformer.cpp -o $OUT/test_host_beamformer $LINK -ldl & pids+=($!); fi
if stale $OUT/test_host_adaptive_weights tests/test_host_adaptive_weights.cpp; then $CXX -O2 tests/test_host_adaptive_weights.cpp -o $OUT/test_host_adaptive_weights $LINK -ldl & pids+=($!); fi
for p in "${pids[@]}"; do wait $p; done
if [ -n "$PLUGIN_OBJS" ]; then $CXX -fPIC -shared -fvisibility=hidden $PLUGIN_OBJS -o ../libgr4hip_blocks.so -L.. -lgr4hip -Wl,-rpath,'$ORIGIN' -Wl,-rpath,/opt/rocm/lib; fi
echo "built $(realpath $OUT)"
