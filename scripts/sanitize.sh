#!/bin/bash
# Sanitizer builds of the host C (the reference builds without any, Makefile:13, and carries
# fifo.c:141,192-197,219).  scripts/sanitize.sh asan|tsan OUTDIR builds, with gcc -fsanitize=address,undefined or
# -fsanitize=thread:
#   OUTDIR/libmsd_host.so   every file of csrc/host/ (FIFO, ifile handler with its reader / consumer threads, wire formats,
#                           converter and demodulator adapters)
#   OUTDIR/libmodes_hip.so  the library's plain-C parts (msd_tables.c, msd_resolve.c with its resolver threads,
#                           msd_fields.c, msd_magbuf.c) instrumented, relinked with the HIP objects of the ordinary build (device code
#                           and its C++ launcher are not gcc's to instrument)
#   OUTDIR/msd_replay       the replay tool
#   OUTDIR/fifo_stress      tests/c/fifo_stress.c: producer twelve buffers ahead, consumer, a halt in mid-stream
#   OUTDIR/aircraft_table_units  tests/c/aircraft_table_units.c: the aircraft table's host twin and msd_aircraft_to_float
#                           under a main of their own; run it as it is
#   OUTDIR/modeac_units     tests/c/modeac_units.c: the Mode A/C matching's host twin and msd_mode_c_to_a, the same way
#   OUTDIR/reduce_units     tests/c/reduce_units.c: the reduced Beast output's host twin, the same way
#   OUTDIR/sbs_units        tests/c/sbs_units.c: the SBS writer's arithmetic (msd_sbs_impl.h, what the device runs) against
#                           snprintf, gmtime_r and atan2, and its lines against the host twin's; asan only, run it as it is
#   OUTDIR/pb_units         tests/c/pb_units.c: the aircraft.pb encoder (msd_pb_impl.h, what the device runs) -- varints,
#                           lengths, the longest entry, the truncating track table -- and its entries against the host twin's;
#                           asan only, run it as it is
#   OUTDIR/vrs_units        tests/c/vrs_units.c: the VRS writer's printing and escaping (msd_vrs_impl.h, what the device
#                           runs) against snprintf, and its objects against the host twin's; asan only, run it as it is
#   OUTDIR/history_units    tests/c/history_units.c: the history_N.pb encoder (msd_history_impl.h, what the device runs) --
#                           every varint length, length == bytes written, the longest entry -- and its entries against the
#                           host twin's; asan only, run it as it is
# Run the python tests against them with MSD_LIBMODES_HIP=OUTDIR/libmodes_hip.so and LD_PRELOAD=$(gcc -print-file-name=libasan.so)
# (tests/test_sanitizers.py does).
set -e
MODE=$1
OUT=$(mkdir -p "$2" && cd "$2" && pwd)
cd "$(dirname "$0")/../readsb-protobuf_amd/csrc"
# asan: gcc (its shared runtime can be preloaded into python).  tsan: the ROCm clang for everything, the C++ stream driver
# (msd_capi.cpp, msd_batch.cpp, msd_collect.cpp) included (hipcc instruments its host side; only the device code is left
# out) -- gcc 11's ThreadSanitizer runtime cannot start on the GPU boxes' kernel ("unexpected memory mapping") and, with the
# driver uninstrumented, takes its own std::mutex / std::atomic hand-overs to the C threads for races.
CC=gcc
CAPI_OBJ="msd_capi.o msd_batch.o msd_collect.o"
case "$MODE" in
asan) SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer"; CXX=g++ ;;
tsan) SAN="-fsanitize=thread -fno-omit-frame-pointer"; CC=/opt/rocm/lib/llvm/bin/clang; CXX=/opt/rocm/lib/llvm/bin/clang++ ;;
*) echo "usage: $0 asan|tsan OUTDIR" >&2; exit 2 ;;
esac
test -f msd_kernels.o -a -f msd_dc_kernels.o -a -f msd_resolve_kernels.o -a -f msd_frames_kernels.o -a -f msd_wire_kernels.o -a -f msd_avr_kernels.o -a -f msd_group_beast_kernels.o -a -f msd_group_avr_kernels.o -a -f msd_group_remote_out_kernels.o -a -f msd_pos_kernels.o -a -f msd_reduce_kernels.o -a -f msd_sbs_kernels.o -a -f msd_pb_kernels.o -a -f msd_vrs_kernels.o -a -f msd_history_kernels.o -a -f msd_range_kernels.o -a -f msd_capi.o -a -f msd_batch.o -a -f msd_collect.o -a -f msd_group.o -a -f msd_frames.o || { echo "run build.sh first (the HIP objects are reused)" >&2; exit 1; }
INC="-I. -I../../include -Ihost"
CF="-std=c11 -O1 -g -Wall -Wextra -fPIC $SAN $INC"
$CC $CF -ffp-contract=off -c msd_tables.c -o "$OUT/msd_tables.o"
$CC $CF -ffp-contract=off -c msd_resolve.c -o "$OUT/msd_resolve.o"
$CC $CF -c msd_fields.c -o "$OUT/msd_fields.o"
$CC $CF -c msd_magbuf.c -o "$OUT/msd_magbuf.o"
if [ "$MODE" = tsan ]; then
    for f in msd_capi msd_batch msd_collect; do
        hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC $SAN -Wno-option-ignored $INC -c $f.cpp -o "$OUT/$f.o"
    done
    CAPI_OBJ="$OUT/msd_capi.o $OUT/msd_batch.o $OUT/msd_collect.o"
fi
# the host side of the Beast / AVR input and the receiver-group driver have no device code: plain host C++ against the
# HIP headers, instrumented in both modes (their kernels stay in msd_frames_kernels.o / msd_kernels.o)
$CXX -std=c++17 -O1 -g -fPIC $SAN -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include $INC -c msd_frames.cpp -o "$OUT/msd_frames.o"
$CXX -std=c++17 -O1 -g -fPIC $SAN -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include $INC -c msd_group.cpp -o "$OUT/msd_group.o"
$CXX -std=c++17 -O1 -g -fPIC $SAN -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include $INC -c msd_group_remote.cpp -o "$OUT/msd_group_remote.o"
$CXX -std=c++17 -O1 -g -fPIC $SAN -ffp-contract=off -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include $INC -c msd_pos.cpp -o "$OUT/msd_pos.o"
CAPI_OBJ="$CAPI_OBJ $OUT/msd_frames.o $OUT/msd_group.o $OUT/msd_group_remote.o $OUT/msd_pos.o"
# (the sanitizer runtime comes from LD_PRELOAD or from the instrumented executable: the shared objects leave it undefined)
# (the wire writers are in both libraries, as in build.sh)
$CC $CF -c host/msd_wire.c -o "$OUT/msd_wire.o"
$CC $CF -ffp-contract=off -c host/msd_receiver_pb.c -o "$OUT/msd_receiver_pb.o"
hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT/libmodes_hip.so" msd_kernels.o msd_dc_kernels.o msd_resolve_kernels.o msd_frames_kernels.o msd_wire_kernels.o msd_avr_kernels.o msd_group_beast_kernels.o msd_group_avr_kernels.o msd_group_remote_out_kernels.o msd_pos_kernels.o msd_reduce_kernels.o msd_sbs_kernels.o msd_pb_kernels.o msd_vrs_kernels.o msd_history_kernels.o msd_range_kernels.o $CAPI_OBJ \
    "$OUT/msd_tables.o" "$OUT/msd_resolve.o" "$OUT/msd_fields.o" "$OUT/msd_magbuf.o" "$OUT/msd_wire.o" "$OUT/msd_receiver_pb.o" -lm -lpthread
for f in msd_fifo msd_sdr_ifile msd_converter msd_demod; do
    $CC $CF -c host/$f.c -o "$OUT/$f.o"
done
$CC $CF -ffp-contract=off -c host/msd_pos_host.c -o "$OUT/msd_pos_host.o"
$CC -shared -fPIC $SAN -o "$OUT/libmsd_host.so" "$OUT"/msd_pos_host.o "$OUT"/msd_fifo.o "$OUT"/msd_sdr_ifile.o "$OUT"/msd_wire.o "$OUT"/msd_receiver_pb.o "$OUT"/msd_converter.o "$OUT"/msd_demod.o \
    -L"$OUT" -lmodes_hip -Wl,-rpath,'$ORIGIN' -lpthread -lm
$CC $CF host/msd_replay_main.c "$OUT"/msd_sdr_ifile.o "$OUT"/msd_fifo.o "$OUT"/msd_wire.o "$OUT"/msd_converter.o -o "$OUT/msd_replay" \
    -L"$OUT" -lmodes_hip -Wl,-rpath,'$ORIGIN' -lpthread -lm
$CC $CF ../../tests/c/fifo_stress.c "$OUT"/msd_fifo.o -o "$OUT/fifo_stress" -lpthread
$CC $CF ../../tests/c/host_units.c "$OUT"/msd_wire.o "$OUT"/msd_tables.o "$OUT"/msd_fields.o "$OUT"/msd_magbuf.o "$OUT"/msd_sdr_ifile.o "$OUT"/msd_fifo.o "$OUT"/msd_converter.o \
    -o "$OUT/host_units" -L"$OUT" -lmodes_hip -Wl,-rpath,'$ORIGIN' -lpthread -lm
# the aircraft table's host twin (msd_trk_impl.h) under its own main: no python, no preload
$CC $CF -ffp-contract=off ../../tests/c/aircraft_table_units.c "$OUT"/msd_pos_host.o "$OUT"/msd_fields.o "$OUT"/msd_tables.o \
    -o "$OUT/aircraft_table_units" -L"$OUT" -lmodes_hip -Wl,-rpath,'$ORIGIN' -lpthread -lm
$CC $CF -ffp-contract=off ../../tests/c/modeac_units.c "$OUT"/msd_pos_host.o "$OUT"/msd_fields.o "$OUT"/msd_tables.o \
    -o "$OUT/modeac_units" -L"$OUT" -lmodes_hip -Wl,-rpath,'$ORIGIN' -lpthread -lm
$CC $CF -ffp-contract=off ../../tests/c/reduce_units.c "$OUT"/msd_pos_host.o "$OUT"/msd_wire.o "$OUT"/msd_fields.o "$OUT"/msd_tables.o \
    -o "$OUT/reduce_units" -L"$OUT" -lmodes_hip -Wl,-rpath,'$ORIGIN' -lpthread -lm
if [ "$MODE" = asan ]; then
    $CC $CF -ffp-contract=off ../../tests/c/sbs_units.c "$OUT"/msd_pos_host.o \
        -o "$OUT/sbs_units" -L"$OUT" -lmodes_hip -Wl,-rpath,'$ORIGIN' -lpthread -lm
    $CC $CF -ffp-contract=off ../../tests/c/pb_units.c "$OUT"/msd_pos_host.o \
        -o "$OUT/pb_units" -L"$OUT" -lmodes_hip -Wl,-rpath,'$ORIGIN' -lpthread -lm
    $CC $CF -ffp-contract=off ../../tests/c/vrs_units.c "$OUT"/msd_pos_host.o \
        -o "$OUT/vrs_units" -L"$OUT" -lmodes_hip -Wl,-rpath,'$ORIGIN' -lpthread -lm
    $CC $CF -ffp-contract=off ../../tests/c/history_units.c "$OUT"/msd_pos_host.o \
        -o "$OUT/history_units" -L"$OUT" -lmodes_hip -Wl,-rpath,'$ORIGIN' -lpthread -lm
fi
echo "sanitizer build ($MODE): $(ls "$OUT" | grep -v '\.o$' | tr '\n' ' ')"
