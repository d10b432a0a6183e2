pair_coeff 1 1 0.09 3.3
pair_coeff 2 2 0.06 3.0
