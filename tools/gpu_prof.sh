# rocprofv3 kernel-trace summaries of the three bench workloads -> $OUT_DIR/${R}prof/*_kernel_stats.csv (OUT_DIR: default prof_out; copy the ones
# to be judged into profiles/).  On an MI355X:  R=r03 bash tools/gpu_prof.sh
cd $GRAFT_REPO_ROOT
R=${R:-r03}
O=${OUT_DIR:-prof_out}/${R}prof
mkdir -p $O
export TMPDIR=/tmp
for wl in mnist nsde latent; do
  rm -rf $O/$wl
  timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/$wl -- python3 bench.py --workload $wl --steps 10 --warmup 3 --full --no-cpu-baseline --no-extras > $O/${wl}_bench.log 2>&1
  tail -1 $O/${wl}_bench.log | cut -c1-300
  head -12 $O/$wl/*/*_kernel_stats.csv | cut -c1-160
  cp $O/$wl/*/*_kernel_stats.csv $O/${wl}_kernel_stats.csv
  find $O/$wl -name "*kernel_trace.csv" -size +20M -delete
done
