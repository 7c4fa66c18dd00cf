set -o pipefail
O=${RPF_OUT:-out}
mkdir -p $O
bash scripts/profile.sh r01h_1080p8 > $O/prof_r01h_1080p8.log 2>&1
BENCH_FLAGS="--width 3840 --rows-per-gpu 270 --spp 32" bash scripts/profile.sh r01h_4k32slab > $O/prof_r01h_4k32slab.log 2>&1
python bench.py --full > $O/bench_r01h.json 2>$O/bench_r01h.err
python bench.py --full --width 3840 --rows-per-gpu 270 --spp 32 --steps 3 --warmup 1 > $O/bench_r01h_4k32slab.json 2>$O/bench_r01h_4k32slab.err
bash scripts/ablate.sh > $O/ablate_r01h.txt 2>&1
bash scripts/sweep.sh > $O/sweep_r01h.txt 2>&1
python scripts/host_path.py 2>&1 | grep -v amdgpu > $O/host_path_r01h.txt
(python scripts/smalln.py; SPP=16 python scripts/smalln.py; SPP=32 ROWS=540 python scripts/smalln.py; SPP=64 ROWS=270 python scripts/smalln.py) 2>&1 | grep -v amdgpu > $O/smalln_r01h.txt
(python scripts/multipass.py 8; python scripts/multipass.py 16; python scripts/multipass.py 32) 2>&1 | grep -v amdgpu > $O/multipass_r01h.txt
tail -2 $O/multipass_r01h.txt
