#!/bin/bash
# One-off on a GPU box: MIOpen solver search for the convolutions of the Mask R-CNN head stand-ins (bench.py --config maskrcnn),
# recorded into $O/miopen_db/ on top of the shipped find-db; copy the .ufdb.txt back into
# panoswintransformerobjectdetection_amd/miopen_db/ afterwards.
# usage: bash tools/miopen_find_heads.sh [output directory, default: a new temporary directory]
set -u
O=${1:-$(mktemp -d)}
mkdir -p $O/miopen_db
cp panoswintransformerobjectdetection_amd/miopen_db/* $O/miopen_db/
export MIOPEN_USER_DB_PATH=$O/miopen_db
export PSWIN_MIOPEN_FIND=1
python bench.py --config maskrcnn --steps 3 --warmup 2 > $O/mr_find.json 2> $O/mr_find.err
echo "find run done: $(tail -c 300 $O/mr_find.json)"
ls -la $O/miopen_db
wc -l $O/miopen_db/*.ufdb.txt
unset PSWIN_MIOPEN_FIND
# --full: the step breakdown printed below is measured only then
python bench.py --config maskrcnn --steps 5 --warmup 2 --full > $O/mr_after.json 2> $O/mr_after.err
python -c "
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print('after', d['value'], d['ms_per_step'], d['step_breakdown_ms'])" $O/mr_after.json
