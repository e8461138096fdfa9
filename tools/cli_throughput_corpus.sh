#!/bin/bash
# End-to-end throughput of cuNVSMTrainModel on the Cranfield fixture (the LSE recipe of tools/cli_throughput.sh) with host batches
# and with --device_corpus (the collection in HBM, batches as 8-byte window references), alternately on one box. Per run it prints
#   cumulative  the trainer's own "batches/second": all batches so far over all time so far, model dumps and the first epoch included;
#   last epoch  n-gram windows/second of the last epoch alone, and the median over all epochs of that per-epoch figure
#               (an epoch of Cranfield is 37 batches, about 10 ms: single epochs are noisy, hence the median and many epochs);
#   costs       a digest of the printed epoch-cost list: the two kinds of run must end on the same one.
# usage: tools/cli_throughput_corpus.sh [epochs] [rounds]
cd "$(dirname "$0")/.."
EPOCHS=${1:-40}
ROUNDS=${2:-2}
for round in $(seq 1 $ROUNDS); do
  for mode in host_batches device_corpus; do
    OUT=$(mktemp -d)
    FLAG=""; [ $mode = device_corpus ] && FLAG="--device_corpus"
    ./cunvsm_amd/bin/cuNVSMTrainModel --word_repr_size 128 --entity_repr_size 256 --window_size 10 --num_random_entities 16 \
        --batch_size 4096 --nonlinearity tanh --bias_negative_samples --update_method full_adam --learning_rate 0.001 \
        --num_epochs $EPOCHS --seed 1 --sampler host --v 1 $FLAG --output $OUT/model tests/golden/cranfield/cranfield.trectext 2> $OUT/log \
        || { echo "round $round $mode: the trainer failed"; tail -5 $OUT/log; rm -rf $OUT; exit 1; }
    COSTS=$(grep -E 'Epoch #[0-9]+: duration' $OUT/log | tail -1 | sed 's/.*cost=//')
    MEDIAN=$(grep 'n-gram windows/second' $OUT/log | sed 's/.*: \([0-9.e+]*\) n-gram.*/\1/' | sort -g | awk '{v[NR]=$1} END {print v[int((NR+1)/2)]}')
    echo "round $round $mode: cumulative $(grep -E 'Epoch #[0-9]+: duration' $OUT/log | tail -1 | sed 's/.*(\(.*batches\/second\)).*/\1/'); last epoch $(grep 'n-gram windows/second' $OUT/log | tail -1 | sed 's/.*: //'); median epoch $MEDIAN windows/second; costs $(echo "$COSTS" | md5sum | cut -c1-8)"
    rm -rf $OUT
  done
done
