#!/usr/bin/env bash
# Developer aid (GPU box): the tail's chunk ring per wave (LMI_RC_SMALL_RING builds under vb/) on the default legs
for lib in learnedmetricindex_amd/liblmi_hip.so vb/ring16.so learnedmetricindex_amd/liblmi_hip.so vb/ring16.so; do
  LMI_LIB=$PWD/$lib timeout -k 10 300 python3 bench.py --full --steps 30 --warmup 6 --no-cpu-baseline --no-recall --no-exact-leg --no-hard-leg 2>/dev/null | python3 -c "
import json,sys;j=json.loads(sys.stdin.read().strip().splitlines()[-1]);o=j['other_configs'];print('$lib', 'c2 step',j['ms_per_step'],'tail',j['phases_ms']['rescore'],'| c1',o['c1']['ms_per_step'],o['c1']['phases_ms']['rescore'],'| c5',o['c5']['ms_per_step'],o['c5']['phases_ms']['rescore'])" || exit 1
done
