pair_coeff 1 1 0.0725 3.31
