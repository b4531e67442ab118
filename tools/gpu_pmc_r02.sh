# HBM traffic of the bench's kernels: two separate --pmc passes (FETCH_SIZE, WRITE_SIZE), as MI355X_MICROARCH.md prescribes
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
O=${OUT_DIR:-prof_out}/r02pmc
mkdir -p $O
for c in FETCH_SIZE WRITE_SIZE; do
  rm -rf $O/$c
  timeout 600 rocprofv3 --kernel-trace --pmc $c --output-format csv -d $O/$c -- python3 bench.py --steps 3 --warmup 1 --full --no-cpu-baseline --no-extras > $O/$c.log 2>&1
  tail -c 300 $O/$c.log
done
python3 tools/pmc_summary.py $O/FETCH_SIZE $O/WRITE_SIZE > $O/r02_pmc_hbm_traffic.csv
cat $O/r02_pmc_hbm_traffic.csv
find $O -name "*.csv" -size +5M -delete
# large per-GPU batch: the same kernels at B = 4096 (roofline at a batch that fills the chip 8 times over)
timeout 900 python3 bench.py --batch 4096 --steps 5 --warmup 2 --full --no-cpu-baseline --no-extras > $O/bench_B4096.json 2> $O/bench_B4096.err
tail -c 2500 $O/bench_B4096.json
