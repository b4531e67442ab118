# HBM traffic of the bench's kernels: two separate --pmc passes (FETCH_SIZE, WRITE_SIZE) with --kernel-trace only, as MI355X_MICROARCH.md
# prescribes -> $OUT_DIR/${R}pmc/${R}_pmc_hbm_traffic.csv (OUT_DIR: default prof_out).   R=r03 bash tools/gpu_pmc.sh
cd $GRAFT_REPO_ROOT
R=${R:-r03}
export TMPDIR=/tmp
O=${OUT_DIR:-prof_out}/${R}pmc
mkdir -p $O
for c in FETCH_SIZE WRITE_SIZE; do
  rm -rf $O/$c
  timeout 600 rocprofv3 --kernel-trace --pmc $c --output-format csv -d $O/$c -- python3 bench.py --steps 3 --warmup 1 --full --no-cpu-baseline --no-extras > $O/$c.log 2>&1
  tail -c 200 $O/$c.log
done
python3 tools/pmc_summary.py $O/FETCH_SIZE $O/WRITE_SIZE > $O/${R}_pmc_hbm_traffic.csv
cat $O/${R}_pmc_hbm_traffic.csv
find $O -name "*.csv" -size +5M -delete
