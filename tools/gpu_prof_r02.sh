# rocprofv3 kernel-trace summaries of the three bench workloads (profiles/r02_*) -> $OUT_DIR/r02prof (OUT_DIR: default prof_out), on an MI355X
cd $GRAFT_REPO_ROOT
O=${OUT_DIR:-prof_out}/r02prof
mkdir -p $O
export TMPDIR=/tmp
for wl in mnist nsde latent; do
  rm -rf $O/$wl
  timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/$wl -- python3 bench.py --workload $wl --steps 10 --warmup 3 --full --no-cpu-baseline --no-extras > $O/${wl}_bench.log 2>&1
  tail -1 $O/${wl}_bench.log | cut -c1-300
  head -16 $O/$wl/*/*_kernel_stats.csv | cut -c1-160
  cp $O/$wl/*/*_kernel_stats.csv $O/${wl}_kernel_stats.csv
  find $O/$wl -name "*kernel_trace.csv" -size +20M -delete
done
