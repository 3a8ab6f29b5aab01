set -e -o pipefail
export HRSEG_COMMIT=$1
bash tools/collect_profiles.sh r04 > gpurun_out/collect.log 2>&1 || { tail -20 gpurun_out/collect.log; exit 1; }
tail -3 gpurun_out/collect.log
cp gpurun_out/profiles_r04/r04_*.csv gpurun_out/profiles_r04/r04_meta.json profiles/
python bench.py --full 2>&1 > profiles/r04_bench_n1.json | tail -2; cut -c1-400 profiles/r04_bench_n1.json
python bench.py --full --model unet --no-cpu-baseline 2>&1 > profiles/r04_bench_unet_n1.json | tail -2; cut -c1-300 profiles/r04_bench_unet_n1.json
python bench.py --full --tree class_tree_tl_extended.json --size 1024 --steps 5 --warmup 2 --no-cpu-baseline --no-probe --no-dedup-line --no-f32-line 2>&1 > profiles/r04_bench_cfg4_geometry_1gpu.json | tail -2; cut -c1-300 profiles/r04_bench_cfg4_geometry_1gpu.json
