#!/bin/bash
# Build libd2t.so for gfx950 in-tree (hipcc cross-compiles without a GPU).
#   bash build.sh                 the shipped library: objects in obj/, libd2t.so
#   D2T_PROBES=1 bash build.sh    a PROBE build (timing-probe / ablation / A-B switches compiled in, read from the environment):
#                                 objects in obj_probe/, libd2t_probe.so -- never libd2t.so.  Tools select it with
#                                 D2T_PROBE_LIB=doc2tex_amd/csrc/libd2t_probe.so (tools/decode_trace.py, tools/probe/*).
set -e
cd "$(dirname "$0")"
OPT="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result -Wno-unused-value -Wno-pass-failed"
OBJ=obj; LIB=libd2t.so
if [ -n "$D2T_PROBES" ]; then OPT="$OPT -DD2T_PROBES"; OBJ=obj_probe; LIB=libd2t_probe.so; fi
mkdir -p $OBJ
SRCS="conv_mfma conv_bf16x3 conv_bf16x3p conv_records ops vit_attn decode decode_gemm decode_row decode_maps decode_beam recurrent attn_beam train_kernels train_wgrad train_attn train_recurrent train train_models train_abi optim optim_family metrics engine engine_weights engine_tfm engine_tfm_beam engine_attn engine_ops prep post posembed"
objs=""; stale=""
for f in $SRCS; do
  o=$OBJ/$f.o
  objs="$objs $o"
  if [ ! -f $o ] || [ $f.hip -nt $o ] || [ kernels.h -nt $o ] || [ conv_common.h -nt $o ] || [ conv_dma.h -nt $o ] || [ train_common.h -nt $o ] || [ train_tape.h -nt $o ] || [ recurrent_common.h -nt $o ] || [ decode_common.h -nt $o ] || [ decode_row_common.h -nt $o ] || [ ctx.h -nt $o ] || [ engine_impl.h -nt $o ] || [ engine_tfm.h -nt $o ] || [ beam_host.h -nt $o ] || [ attn_beam_host.h -nt $o ] || [ carve.h -nt $o ] || [ optim_common.h -nt $o ] || [ ../../include/d2t.h -nt $o ] || [ ../../include/d2t_prep.h -nt $o ] || [ unicode_tables.h -nt $o ] || [ build.sh -nt $o ]; then
    stale="$stale $f"
  fi
done
# at most 16 compilers at a time; set -e: a failed compile fails the build (xargs returns 123; no stale object is linked)
if [ -n "$stale" ]; then
  printf '%s\n' $stale | xargs -P 16 -I{} sh -c "hipcc $OPT -c {}.hip -o $OBJ/{}.o.tmp && mv $OBJ/{}.o.tmp $OBJ/{}.o"
fi
hipcc --offload-arch=gfx950 -shared -fPIC -o $LIB $objs
echo "built $(pwd)/$LIB"
