L=$(mktemp); J=$(mktemp)
for cfg in "4,14,4,7,16,14,16,14" "4,14,4,7,16,14,8,14" "4,14,4,7,8,14,16,14" "2,14,4,7,16,14,16,14" "4,14,4,15,16,14,16,14" "4,14,3,10,16,14,16,14" "4,10,4,7,16,14,16,10" "3,14,4,7,12,14,12,14"; do
  echo "== $cfg"; BSX_SEG_TILES=$cfg python bench.py --full --no-extra-configs --no-cpu-baseline --steps 10 --dump-launches $L > $J 2>/dev/null; grep -E "seg_|frame_program" $L | awk '{printf "%s %s  ", $2, $3}'; python -c "import json, sys; d=json.load(open(sys.argv[1])); print(' fps', d['value'])" $J
done
rm -f $L $J
